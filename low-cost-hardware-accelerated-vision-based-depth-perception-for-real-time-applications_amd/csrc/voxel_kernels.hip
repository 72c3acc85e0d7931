// Voxel-grid downsampled clouds from disparity maps: one row per occupied cell of a regular 3-D grid - centroid, mean colour, number of
// points -, fused with the reprojection and with (F)'s selection (no list of points is written).  Specified in
// include/stereo_vision_hip.h (I), restated in stereo_vision/sv.py: voxel_cloud.
//
//   kept      (F)'s predicate, cloud_run of cloud_kernels.h, one visited pixel per lane (a tile is CLOUD_TILE visited pixels and one
//             wavefront, as there)
//   cell      per axis t = (P - lo) / size, c = min((int64)t, n - 1), u = min((int64)((t - c) * 65536), 65535); key = c_x | c_y << 20 |
//             c_z << 40 < 2^60, so the all-ones word is free to mean "empty"
//   table     per pair, open addressing with linear probing, `slots` (a power of two >= 2 * capacity) entries of nine 64-bit words:
//             key | first, n | S[3] | C[4].  An entry only ever meets integer atomics whose result does not depend on their order (CAS on
//             the key, min on first, add on the rest), so a pair's table holds the same values whatever the schedule was; WHERE an entry
//             lies does depend on it, and nothing that is written out does.
//   widths    n and first are 32 bits (a frame has < 2^31 visited pixels); S_k <= 65535 n < 2^47 and C_j <= 255 n < 2^39 are 64 bits; the
//             partial sums of a wavefront's run (<= 64 points) are < 2^22 and < 2^14 and travel as 32 and 16 bits
//   clear     key and first all ones, everything else - head, mask - zero, 16 bytes per thread
//   insert    a claim (the CAS that turns an empty key into ours) counts into the pair's head; the claim that exceeds the capacity marks
//             the pair overflowed, and wavefronts that see the mark stop.  A probe sequence is bounded by `slots`; a lane never waits
//             for another one: a CAS that finds someone else's key moves on.  With `combine` the lanes of a wavefront are split into
//             runs of equal keys (neighbouring pixels mostly share a cell) and the last lane of a run updates the table with the run's
//             sums from a segmented scan; n and first follow from the run's length, since the lanes' pixels are consecutive.
//   mark      an occupied slot sets the bit of its first visited pixel in the pair's mask: that pixel owns the voxel's row
//   count     tiles[b][t] = set bits of tile t; (F)'s k_cloud_scan turns them into offsets
//   write     one wavefront per tile, a lane per 16 mask bits: rank from a shuffle scan, then per owner pixel the point again, its
//             key, the entry (plain loads: a kernel boundary lies between), the row
//
// Every load of the map is guarded by v < n_visited (cloud_run), every store by row < capacity, every mask access by its word < n_words,
// every slot index is masked by slots - 1; a tile index is < n_tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

constexpr unsigned long long VOXEL_EMPTY = ~0ull;

struct PairWs {
    unsigned long long *table;
    uint32_t *head;  // [0] claimed slots, [1] overflowed
    uint32_t *mask;
};

__device__ __forceinline__ PairWs pair_ws(const VoxelArgs &a, int b) {
    uint8_t *p = a.ws + (size_t)b * a.pair_bytes;
    PairWs w;
    w.table = reinterpret_cast<unsigned long long *>(p);
    w.head = reinterpret_cast<uint32_t *>(p + a.mask_offset - VOXEL_HEAD_BYTES);
    w.mask = reinterpret_cast<uint32_t *>(p + a.mask_offset);
    return w;
}

__device__ __forceinline__ uint32_t overflowed(const uint32_t *head) { return __hip_atomic_load(head + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t slot_of(const VoxelArgs &a, unsigned long long key) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - a.log2_slots));  // log2_slots in 10 .. 27
}

// The cell and the offsets inside it of a kept point (lo < P < hi, all finite): the header's arithmetic, in its order.
__device__ __forceinline__ unsigned long long voxel_key(const VoxelArgs &a, const double *P, uint32_t *u) {
    unsigned long long key = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double t = (P[k] - a.c.lo[k]) / a.size;
        long long c = (long long)t;
        if (c > a.nc[k] - 1) c = a.nc[k] - 1;
        long long o = (long long)((t - (double)c) * 65536.0);
        if (o > 65535) o = 65535;
        u[k] = (uint32_t)o;
        key |= (unsigned long long)c << (20 * k);
    }
    return key;
}

__global__ __launch_bounds__(256) void k_voxel_clear(VoxelArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // 16-byte unit of the pair
    if (i * 16 >= a.pair_bytes) return;
    const size_t table_words = ((size_t)1 << a.log2_slots) * VOXEL_ENTRY_WORDS;
    unsigned long long w[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const size_t word = 2 * i + k;
        const unsigned r = (unsigned)(word % VOXEL_ENTRY_WORDS);
        w[k] = word < table_words ? (r == 0 ? VOXEL_EMPTY : (r == 1 ? 0xFFFFFFFFull : 0ull)) : 0ull;
    }
    *reinterpret_cast<ulonglong2 *>(a.ws + (size_t)blockIdx.y * a.pair_bytes + i * 16) = make_ulonglong2(w[0], w[1]);
}

// Adds a run (n points, the first at visited pixel `first`, offset sums S, colour sums C) to the voxel `key` of the pair.
template <bool COUNT_ATOMICS>
__device__ __forceinline__ void voxel_add(const VoxelArgs &a, const PairWs &w, unsigned long long key, uint32_t n, uint32_t first, const uint32_t *S,
                                          const uint32_t *C, bool colors) {
    const uint32_t last = (uint32_t)(((size_t)1 << a.log2_slots) - 1);
    uint32_t h = slot_of(a, key), issued = 0;
    for (uint32_t probe = 0; probe <= last; probe++, h = (h + 1) & last) {
        if ((probe & 15) == 15 && overflowed(w.head)) break;  // a full table of a pair that is lost anyway
        unsigned long long *e = w.table + (size_t)h * VOXEL_ENTRY_WORDS;
        const unsigned long long old = atomicCAS(e, VOXEL_EMPTY, key);
        issued++;
        if (old == VOXEL_EMPTY) {  // claimed
            issued++;
            if (atomicAdd(w.head, 1u) >= (uint32_t)a.c.capacity) atomicOr(w.head + 1, 1u), issued++;
        } else if (old != key) {
            continue;  // someone else's: the next slot
        }
        uint32_t *fn = reinterpret_cast<uint32_t *>(e + 1);
        atomicMin(fn, first);
        atomicAdd(fn + 1, n);
#pragma unroll
        for (int k = 0; k < 3; k++) atomicAdd(e + 2 + k, (unsigned long long)S[k]);
        if (colors) {
#pragma unroll
            for (int j = 0; j < 4; j++) atomicAdd(e + 5 + j, (unsigned long long)C[j]);
        }
        issued += colors ? 9 : 5;
        if (COUNT_ATOMICS) atomicAdd(a.counters, 1ull), atomicAdd(a.counters + 1, (unsigned long long)issued);
        return;
    }
    atomicOr(w.head + 1, 1u);  // no slot within `slots` probes: more voxels than the capacity
    if (COUNT_ATOMICS) atomicAdd(a.counters + 1, (unsigned long long)issued + 1);
}

template <int SRC, bool COMBINE, bool COUNT_ATOMICS>
__global__ __launch_bounds__(64 * CLOUD_WAVES) void k_voxel_insert(VoxelArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int tile = blockIdx.x * CLOUD_WAVES + (threadIdx.x >> 6);
    if (tile >= a.c.n_tiles) return;  // the whole wavefront
    const PairWs w = pair_ws(a, b);
    const float *frame = a.c.disp + (size_t)b * a.c.W * a.c.H;
    const bool colors = a.c.colors != nullptr;
    for (int s = 0; s < CLOUD_TILE / 64; s++) {
        if (__shfl(overflowed(w.head), 0)) return;  // the whole wavefront: the pair's rows mean nothing any more
        const uint32_t v = (uint32_t)tile * CLOUD_TILE + (uint32_t)(s * 64 + lane);
        int pix;
        double P[1][3];
        const bool keep = cloud_run<SRC, 1>(a.c, frame, false, v, &pix, P) != 0u;
        unsigned long long key = VOXEL_EMPTY;
        uint32_t S[3] = {0u, 0u, 0u}, C[4] = {0u, 0u, 0u, 0u}, n = 1, first = v;
        if (keep) {
            key = voxel_key(a, P[0], S);
            if (colors) {
                const uint32_t c = reinterpret_cast<const uint32_t *>(a.c.colors)[(size_t)b * a.c.W * a.c.H + pix];
                C[0] = c & 255u, C[1] = (c >> 8) & 255u, C[2] = (c >> 16) & 255u, C[3] = c >> 24;
            }
        }
        bool issue = keep;
        if (COMBINE) {  // every lane of the wavefront gets here
            const WaveRun run = wave_run(key);
            uint32_t c01 = C[0] | (C[1] << 16), c23 = C[2] | (C[3] << 16);  // a run's sums are <= 64 * 255 < 2^16
            wave_run_scan(run, [&](int d, bool take) {  // the tail holds the run's sums
                const uint32_t s0 = __shfl_up(S[0], d), s1 = __shfl_up(S[1], d), s2 = __shfl_up(S[2], d);
                const uint32_t t01 = colors ? __shfl_up(c01, d) : 0u, t23 = colors ? __shfl_up(c23, d) : 0u;
                if (take) S[0] += s0, S[1] += s1, S[2] += s2, c01 += t01, c23 += t23;
            });
            C[0] = c01 & 0xFFFFu, C[1] = c01 >> 16, C[2] = c23 & 0xFFFFu, C[3] = c23 >> 16;
            n = (uint32_t)(lane - run.head_lane + 1);  // the run's lanes hold consecutive visited pixels, all kept
            first = v - (n - 1);
            issue = keep && run.tail;
        }
        if (issue) voxel_add<COUNT_ATOMICS>(a, w, key, n, first, S, C, colors);
    }
}

__global__ __launch_bounds__(256) void k_voxel_mark(VoxelArgs a) {
    const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= ((size_t)1 << a.log2_slots)) return;
    const PairWs w = pair_ws(a, blockIdx.y);
    if (w.head[1]) return;  // overflowed: no owners, no rows
    const unsigned long long *e = w.table + h * VOXEL_ENTRY_WORDS;
    if (e[0] == VOXEL_EMPTY) return;
    const uint32_t first = (uint32_t)e[1];
    if (first < (uint32_t)a.c.n_visited) atomicOr(w.mask + (first >> 5), 1u << (first & 31));  // always true for an occupied slot
}

__global__ __launch_bounds__(256) void k_voxel_count(VoxelArgs a) {
    const int tile = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (tile >= a.c.n_tiles) return;
    const uint32_t *mask = pair_ws(a, b).mask;
    int total = 0;
    for (int q = 0; q < CLOUD_TILE / 128; q++) {
        const int word = tile * (CLOUD_TILE / 32) + q * 4;  // the mask is padded to four words and the padding is zero
        if (word < a.n_words) {
            const uint4 m = *reinterpret_cast<const uint4 *>(mask + word);
            total += __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
        }
    }
    a.c.tiles[(size_t)b * a.c.n_tiles + tile] = total;
}

template <int SRC, int DT>
__global__ __launch_bounds__(64 * CLOUD_WAVES) void k_voxel_write(VoxelArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int tile = blockIdx.x * CLOUD_WAVES + (threadIdx.x >> 6);
    if (tile >= a.c.n_tiles) return;  // the whole wavefront
    const PairWs w = pair_ws(a, b);
    if (w.head[1]) {  // the scan kernel stored 0 for the empty mask
        if (tile == 0 && lane == 0) a.c.counts[b] = -1;
        return;
    }
    const int word = tile * (CLOUD_TILE / 32) + (lane >> 1);
    uint32_t bits = word < a.n_words ? (w.mask[word] >> (16 * (lane & 1))) & 0xFFFFu : 0u;
    const int own = __popc(bits);
    int r = a.c.tiles[(size_t)b * a.c.n_tiles + tile] + wave_inclusive_sum(own) - own;
    const float *frame = a.c.disp + (size_t)b * a.c.W * a.c.H;
    const uint32_t last = (uint32_t)(((size_t)1 << a.log2_slots) - 1);
    for (; bits; bits &= bits - 1, r++) {
        const uint32_t v = (uint32_t)tile * CLOUD_TILE + (uint32_t)lane * 16 + (uint32_t)(__ffs(bits) - 1);
        int pix;
        double P[1][3];
        if (!cloud_run<SRC, 1>(a.c, frame, false, v, &pix, P) || r >= a.c.capacity) continue;  // neither happens for an owner
        uint32_t u[3];
        const unsigned long long key = voxel_key(a, P[0], u);
        uint32_t h = slot_of(a, key);
        const unsigned long long *e = nullptr;
        for (uint32_t probe = 0; probe <= last; probe++, h = (h + 1) & last) {
            const unsigned long long *c = w.table + (size_t)h * VOXEL_ENTRY_WORDS;
            const unsigned long long k = c[0];
            if (k == key) e = c;
            if (k == key || k == VOXEL_EMPTY) break;
        }
        if (!e) continue;  // an owner's voxel is in the table
        const uint32_t n = (uint32_t)(e[1] >> 32);
        const size_t o = (size_t)b * a.c.capacity + (size_t)r;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double c = (double)(long long)((key >> (20 * k)) & 0xFFFFFull);
            const double m = a.c.lo[k] + (c + ((double)e[2 + k] + 0.5 * (double)n) / (65536.0 * (double)n)) * a.size;
            if (DT == CLOUD_F32) static_cast<float *>(a.c.xyz)[3 * o + k] = (float)m;
            else static_cast<double *>(a.c.xyz)[3 * o + k] = m;
            if (a.cell_out) a.cell_out[3 * o + k] = (int32_t)((key >> (20 * k)) & 0xFFFFFull);
        }
        if (a.n_out) a.n_out[o] = (int32_t)n;
        if (a.first_out) a.first_out[o] = pix;
        if (a.c.color_out) {
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) c |= (uint32_t)((2ull * e[5 + j] + n) / (2ull * n)) << (8 * j);  // <= 255
            reinterpret_cast<uint32_t *>(a.c.color_out)[o] = c;
        }
    }
}

dim3 tile_grid(const VoxelArgs &a, int batch) { return dim3((a.c.n_tiles + CLOUD_WAVES - 1) / CLOUD_WAVES, batch); }

template <int SRC>
hipError_t launch_insert_src(bool combine, const VoxelArgs &a, int batch, hipStream_t st) {
    const dim3 grid = tile_grid(a, batch), block(64 * CLOUD_WAVES);
    if (combine) {
        if (a.counters) hipLaunchKernelGGL((k_voxel_insert<SRC, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_voxel_insert<SRC, true, false>), grid, block, 0, st, a);
    } else {
        if (a.counters) hipLaunchKernelGGL((k_voxel_insert<SRC, false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_voxel_insert<SRC, false, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

template <int SRC>
hipError_t launch_write_src(int dtype, const VoxelArgs &a, int batch, hipStream_t st) {
    if (dtype == CLOUD_F32)
        hipLaunchKernelGGL((k_voxel_write<SRC, CLOUD_F32>), tile_grid(a, batch), dim3(64 * CLOUD_WAVES), 0, st, a);
    else if (dtype == CLOUD_F64)
        hipLaunchKernelGGL((k_voxel_write<SRC, CLOUD_F64>), tile_grid(a, batch), dim3(64 * CLOUD_WAVES), 0, st, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

hipError_t launch_voxel_clear(const VoxelArgs &a, int batch, hipStream_t st) {
    const size_t units = a.pair_bytes / 16;  // < 2^32 threads: slots <= 2^27
    hipLaunchKernelGGL(k_voxel_clear, dim3((unsigned)((units + 255) / 256), batch), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_insert(int src, bool combine, const VoxelArgs &a, int batch, hipStream_t st) {
    if (src == CLOUD_SRC_DMAP) return launch_insert_src<CLOUD_SRC_DMAP>(combine, a, batch, st);
    if (src == CLOUD_SRC_D1) return launch_insert_src<CLOUD_SRC_D1>(combine, a, batch, st);
    return hipErrorInvalidValue;
}

hipError_t launch_voxel_mark(const VoxelArgs &a, int batch, hipStream_t st) {
    const size_t slots = (size_t)1 << a.log2_slots;
    hipLaunchKernelGGL(k_voxel_mark, dim3((unsigned)((slots + 255) / 256), batch), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_count(const VoxelArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_voxel_count, dim3((a.c.n_tiles + 255) / 256, batch), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_write(int src, int dtype, const VoxelArgs &a, int batch, hipStream_t st) {
    if (src == CLOUD_SRC_DMAP) return launch_write_src<CLOUD_SRC_DMAP>(dtype, a, batch, st);
    if (src == CLOUD_SRC_D1) return launch_write_src<CLOUD_SRC_D1>(dtype, a, batch, st);
    return hipErrorInvalidValue;
}

}  // namespace sv
