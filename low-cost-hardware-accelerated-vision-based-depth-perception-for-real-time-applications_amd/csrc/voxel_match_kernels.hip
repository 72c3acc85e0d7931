// A frame's rows matched against the world-fixed voxel map over candidate 3-D poses: include/stereo_vision_hip.h (R), restated in
// stereo_vision/sv.py (voxel_map_match).  The map's buffer is voxel_map_kernels.h's and is only read; the row's way into a cell, the
// probe and the filters are voxel_map_table.h's.  Three kernels, no atomics, and no workgroup waits for another:
//
//   scores  grid (row chunk, candidate group, frame).  A lane holds VMATCH_ROWS rows of its frame - x, y, z widened to double, and w -
//           in registers; the workgroup walks its group's candidates, whose twelve pose words every lane reads from the same address (a
//           scalar load).  Per row and candidate: voxel_map_insert's transform in double and in its order, its real division by `size`,
//           the cell, the offsets and the key; a read-only linear probe from slot_of(key) that ends at the key, at an empty key or after
//           `slots` probes - plain loads: a kernel boundary lies behind the insert -; on a hit the three filters, the 64-bit S / n and the
//           squares.  A lane adds up its rows; the wavefront's sums (wave_ops.h) go to the wavefront's own cells of an LDS array - a
//           wavefront no row of which was kept under the candidate skips that -, and behind the last tile the four wavefronts' cells are
//           added and stored as the chunk's partial: [frame][chunk][plane][candidate], planes inside | hits << 32, weight, d2.  A frame
//           of more than VMATCH_MAX_CHUNKS tiles gives a workgroup several tiles, VMATCH_MAX_CHUNKS apart, so the partials stay bounded.
//           Chunks beyond the frame's rows, and every chunk of an overflowed map, store nothing: the sum kernel knows which they are.
//   sums    a lane per candidate adds the partials of the chunks that have rows and stores the four outputs; the workgroup's best goes
//           to the workspace as (weight, d2, index).
//   best    a workgroup per frame over its at most VMATCH_GROUPS bests.
//
// widths    a row's weight is below 2^31 and a frame has fewer than 2^31 rows: inside and hits fit 31 bits each and share a word, and
//           weight < 2^62.  A row adds at most 3 * 65535^2 < 2^34 to d2: below 2^60 for the frames of (I) and (F), which have at most
//           2^26 rows (with more the sum may wrap, as the definition's int64 does).
//
// Every load of a row is guarded by row < min(counts[b], cap), every slot index is masked by slots - 1, every candidate index is < P.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "voxel_map_table.h"
#include "voxel_match_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

// The rows frame b has: min(counts[b], cap), 0 for a count below 1.
__device__ __forceinline__ int rows_of(const VoxelMatchArgs &a, int b) {
    const int cnt = vmap_rows_of(a.counts, b, a.cap);
    return cnt > 0 ? cnt : 0;
}

template <int DT>
__global__ __launch_bounds__(VMATCH_THREADS) void k_vmatch_scores(VoxelMatchArgs a) {
    __shared__ unsigned long long s_acc[VMATCH_THREADS / 64][1 << VMATCH_MAX_LOG_GROUP][VMATCH_PLANES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (int)blockIdx.x, b = (int)blockIdx.z;
    const int p0 = (int)blockIdx.y << a.log_group;                                    // < P
    const int np = a.P - p0 < (1 << a.log_group) ? a.P - p0 : (1 << a.log_group);  // candidates of this workgroup, >= 1
    const int rows = rows_of(a, b);
    if (vmap_overflowed_before(a.map) || (long long)chunk * VMATCH_TILE >= rows) return;  // the whole workgroup
    for (int i = tid; i < (VMATCH_THREADS / 64 << VMATCH_MAX_LOG_GROUP) * VMATCH_PLANES; i += VMATCH_THREADS) (&s_acc[0][0][0])[i] = 0ull;
    __syncthreads();
    const unsigned long long *table = vmap_table(a.map);

    for (long long tile = chunk; tile * VMATCH_TILE < rows; tile += a.n_chunks) {  // the same trips for every thread
        double x[VMATCH_ROWS], y[VMATCH_ROWS], z[VMATCH_ROWS];
        int wt[VMATCH_ROWS];
#pragma unroll
        for (int r = 0; r < VMATCH_ROWS; r++) {
            const long long i = tile * VMATCH_TILE + r * VMATCH_THREADS + tid;
            x[r] = y[r] = z[r] = 0.0, wt[r] = 0;  // a weight of 0: not kept
            if (i < rows) {
                const size_t o = (size_t)b * a.cap + (size_t)i;
                vmap_load_row<DT>(a.xyz, o, x[r], y[r], z[r]);
                wt[r] = a.weight ? a.weight[o] : 1;
            }
        }
        for (int c = 0; c < np; c++) {
            const double *pose = a.poses + ((size_t)b * a.P + (size_t)(p0 + c)) * 12;  // the same address in every lane
            unsigned long long cnt = 0, wsum = 0, dsum = 0;
#pragma unroll
            for (int r = 0; r < VMATCH_ROWS; r++) {
                bool keep = wt[r] > 0;
                unsigned long long key = 0;
                long long u[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    double t;
                    long long cell;
                    keep = vmap_cell(a, pose, k, x[r], y[r], z[r], keep, t, cell);
                    u[k] = vmap_offset(t, cell);
                    key |= vmap_key_part(cell, k);
                }
                if (!keep) continue;
                cnt += 1ull;
                const long long at = vmap_find(table, a.log2_slots, key);
                if (at < 0) continue;
                const unsigned long long *e = table + (size_t)at * VMAP_ENTRY_WORDS;
                const unsigned long long n = e[VMAP_N];
                if (!vmap_passes(a, e) || n == 0ull) continue;
                cnt += 1ull << 32;
                wsum += (unsigned long long)wt[r];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const long long d = u[k] - (long long)(e[VMAP_S + k] / n);
                    dsum += (unsigned long long)(d * d);
                }
            }
            if (!__ballot(cnt != 0ull)) continue;  // the whole wavefront: nothing kept under this candidate
            cnt = wave_sum(cnt), wsum = wave_sum(wsum), dsum = wave_sum(dsum);
            if (lane == 0) s_acc[wave][c][0] += cnt, s_acc[wave][c][1] += wsum, s_acc[wave][c][2] += dsum;
        }
    }
    __syncthreads();
    if (tid < np) {
        unsigned long long *out = a.partials + ((size_t)b * a.n_chunks + (size_t)chunk) * VMATCH_PLANES * (size_t)a.P + (size_t)(p0 + tid);
#pragma unroll
        for (int j = 0; j < VMATCH_PLANES; j++) {
            unsigned long long v = 0;
#pragma unroll
            for (int w = 0; w < VMATCH_THREADS / 64; w++) v += s_acc[w][tid][j];
            out[(size_t)j * a.P] = v;
        }
    }
}

// The larger weight, then the smaller d2, then the lower index.
__device__ __forceinline__ bool better(long long w, long long d, int i, long long w0, long long d0, int i0) {
    return w > w0 || (w == w0 && (d < d0 || (d == d0 && i < i0)));
}

// The best of the workgroup's triples, in thread 0's cells.  Every thread gets here.
__device__ __forceinline__ void block_best(long long *s_w, long long *s_d, int *s_i, long long w, long long d, int i) {
    const int tid = (int)threadIdx.x;
    s_w[tid] = w, s_d[tid] = d, s_i[tid] = i;
    for (int s = VMATCH_THREADS >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s && better(s_w[tid + s], s_d[tid + s], s_i[tid + s], s_w[tid], s_d[tid], s_i[tid]))
            s_w[tid] = s_w[tid + s], s_d[tid] = s_d[tid + s], s_i[tid] = s_i[tid + s];
    }
    __syncthreads();
}

__global__ __launch_bounds__(VMATCH_THREADS) void k_vmatch_sums(VoxelMatchArgs a) {
    __shared__ long long s_w[VMATCH_THREADS], s_d[VMATCH_THREADS];
    __shared__ int s_i[VMATCH_THREADS];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y, p = (int)blockIdx.x * VMATCH_GROUPS + tid;
    const int rows = rows_of(a, b);
    const int tiles = (int)(((long long)rows + VMATCH_TILE - 1) / VMATCH_TILE);
    const int live = vmap_overflowed_before(a.map) ? 0 : (tiles < a.n_chunks ? tiles : a.n_chunks);  // the chunks whose partials were stored
    unsigned long long cnt = 0, wsum = 0, dsum = 0;
    if (p < a.P) {
        const unsigned long long *in = a.partials + (size_t)b * a.n_chunks * VMATCH_PLANES * (size_t)a.P + (size_t)p;
        for (int c = 0; c < live; c++, in += (size_t)VMATCH_PLANES * a.P) cnt += in[0], wsum += in[a.P], dsum += in[2 * (size_t)a.P];
        if (a.inside) {
            const size_t o = (size_t)b * a.P + (size_t)p;
            a.inside[o] = (int32_t)(uint32_t)cnt, a.hits[o] = (int32_t)(cnt >> 32);
            a.weight_out[o] = (long long)wsum, a.d2[o] = (long long)dsum;
        }
    }
    block_best(s_w, s_d, s_i, p < a.P ? (long long)wsum : LLONG_MIN, (long long)dsum, p < a.P ? p : INT_MAX);
    if (tid == 0) {  // candidate blockIdx.x * VMATCH_GROUPS exists, so the triple is one
        VoxelMatchBest *out = a.bests + (size_t)b * VMATCH_GROUPS + blockIdx.x;
        out->weight = s_w[0], out->d2 = s_d[0], out->index = s_i[0], out->pad = 0;
    }
}

__global__ __launch_bounds__(VMATCH_THREADS) void k_vmatch_best(VoxelMatchArgs a) {
    __shared__ long long s_w[VMATCH_THREADS], s_d[VMATCH_THREADS];
    __shared__ int s_i[VMATCH_THREADS];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int groups = (a.P + VMATCH_GROUPS - 1) / VMATCH_GROUPS;  // <= VMATCH_GROUPS
    const VoxelMatchBest *in = a.bests + (size_t)b * VMATCH_GROUPS;
    const bool live = tid < groups;
    block_best(s_w, s_d, s_i, live ? in[tid].weight : LLONG_MIN, live ? in[tid].d2 : 0ll, live ? in[tid].index : INT_MAX);
    if (tid == 0) {
        const bool over = vmap_overflowed_before(a.map);
        a.best[b] = over ? -1 : s_i[0], a.best_weight[b] = over ? 0ll : s_w[0], a.best_d2[b] = over ? 0ll : s_d[0];
    }
}

}  // namespace

hipError_t launch_voxel_match(int dtype, const VoxelMatchArgs &a, hipStream_t st) {
    if (dtype != VMAP_F32 && dtype != VMAP_F64) return hipErrorInvalidValue;
    const dim3 block(VMATCH_THREADS);
    if (a.cap > 0) {
        const dim3 grid((unsigned)a.n_chunks, (unsigned)((a.P + (1 << a.log_group) - 1) >> a.log_group), (unsigned)a.B);
        if (dtype == VMAP_F32) hipLaunchKernelGGL(k_vmatch_scores<VMAP_F32>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_vmatch_scores<VMAP_F64>, grid, block, 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    hipLaunchKernelGGL(k_vmatch_sums, dim3((unsigned)((a.P + VMATCH_GROUPS - 1) / VMATCH_GROUPS), (unsigned)a.B), block, 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    hipLaunchKernelGGL(k_vmatch_best, dim3((unsigned)a.B), block, 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
