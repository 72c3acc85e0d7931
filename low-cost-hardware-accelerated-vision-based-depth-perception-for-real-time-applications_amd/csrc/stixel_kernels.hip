// Stixels and detector-free object boxes from disparity maps and obstacle labels, for a batch.  Specified in
// include/stereo_vision_hip.h (H), restated in stereo_vision/sv.py (stixels, stixel_objects).
//
//   bin       foreground iff label == 2, d > 0 and q >= q_min; q = min(rintf(4.0f * d), n_bins - 1): the only floating-point operations
//             of this file, both exact
//   columns   k_stixel_columns: a lane per visited column walks from the bottom row upwards, one row per trip of ONE loop that is either
//             outside a run or inside one; the run's base bin, first row, last matching row, matching rows and current gap sit in
//             registers.  A run that ends steps back to the row above its last match - at most max_gap + 1 rows are read twice -, so
//             the lanes of a wavefront drift apart by the rows they re-read; they start on one row (64 neighbouring floats and 64 label
//             bytes per load with col_step 1).  A finished stixel is one 16-byte store; the -1 of the unused layers are written at the
//             end of the walk, so nothing has to be cleared beforehand.  The first layer also goes to the workspace, which is what the
//             second kernel reads: it does not depend on the stixels output being asked for.
//   objects   k_stixel_objects: a workgroup per pair, the visited columns in chunks of STIXEL_THREADS with carried prefixes.  A thread
//             per column flags "a segment starts here" and "a segment ends here" from the first layer of the columns i - 1, i, i + 1.  A
//             running maximum of the start positions (wave_ops.h's wave_inclusive_max, wave totals through LDS, the carry from the chunk before)
//             tells the column that ends a segment where it began; a prefix sum over "ends a kept segment" gives the segment its output
//             row.  The kept segments of a chunk are queued in LDS and taken by the four wavefronts in turn: 64 lanes stride over the
//             segment's columns for top, bottom, q_lo, q_hi (wave_min / wave_max), then find the lower median by bisection on the value - at most
//             12 counting passes over q_lo .. q_hi.  A rank count, not an LDS histogram per segment: a segment of a few columns would
//             pay for clearing up to 4096 bins, four of them would have to sit side by side, and the passes read 16 bytes per column
//             that the cache holds.  No atomics anywhere, no workgroup waits for another.
//
// Every load and store is guarded: a visited column i < Wv (so u = i * col_step < W), a row 0 <= v < H, a layer < max_layers, an output
// row < capacity; layer0 is written for every i < Wv by the first kernel before the second reads it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stixel_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

__global__ __launch_bounds__(STIXEL_COLUMNS) void k_stixel_columns(StixelArgs a) {
    const unsigned iu = blockIdx.x * (unsigned)STIXEL_COLUMNS + threadIdx.x;  // unsigned: Wv may be within 64 of 2^31
    if (iu >= (unsigned)a.Wv) return;
    const int b = blockIdx.y, i = (int)iu;
    const size_t u = (size_t)i * a.col_step;  // < W
    const float *col = a.disp + (size_t)b * a.H * a.W + u;
    const uint8_t *lab = a.labels + (size_t)b * a.H * a.W + u;
    int4 *out = a.stixels ? a.stixels + (size_t)b * a.max_layers * a.Wv + i : nullptr;  // layer k at out[k * Wv]
    const float top = (float)(a.n_bins - 1);
    const int4 none = make_int4(-1, -1, -1, -1);
    int4 first = none;
    int count = 0;
    bool in_run = false;
    int qb = 0, vb = 0, t = 0, n = 0, gap = 0;
    int v = a.H - 1;
    for (;;) {
        bool ends = false;
        if (v >= 0) {
            const float d = col[(size_t)v * a.W];
            int q = -1;  // not foreground
            if (lab[(size_t)v * a.W] == 2 && d > 0.f) {
                q = (int)fminf(rintf(4.0f * d), top);
                if (q < a.q_min) q = -1;
            }
            if (!in_run) {
                if (q >= 0) in_run = true, qb = q, vb = v, t = v, n = 1, gap = 0;
                v--;
            } else {
                const int e = q - qb;
                if (q >= 0 && (e < 0 ? -e : e) <= a.sim) {
                    t = v, n++, gap = 0;
                    v--;
                } else if (++gap > a.max_gap) {
                    ends = true;
                } else {
                    v--;
                }
            }
        } else if (in_run) {
            ends = true;  // the image top
        } else {
            break;
        }
        if (ends) {
            if (n >= a.min_rows) {
                const int4 s = make_int4(vb, t, qb, n);
                if (count == 0) first = s;
                if (out && count < a.max_layers) out[(size_t)count * a.Wv] = s;
                count++;
            }
            in_run = false;
            v = t - 1;  // the rows above t that only ended the run are visited again
        }
    }
    if (out)
        for (int k = count; k < a.max_layers; k++) out[(size_t)k * a.Wv] = none;
    if (a.n_stixels) a.n_stixels[(size_t)b * a.Wv + i] = count;
    a.layer0[(size_t)b * a.Wv + i] = first;
}

__global__ __launch_bounds__(STIXEL_THREADS) void k_stixel_objects(StixelArgs a) {
    constexpr int WAVES = STIXEL_THREADS / 64;
    __shared__ int s_start[WAVES], s_kept[WAVES];
    __shared__ int s_first[STIXEL_THREADS], s_last[STIXEL_THREADS];  // the chunk's kept segments that have an output row, in order
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int4 *L = a.layer0 + (size_t)b * a.Wv;
    int4 *boxes = a.boxes ? a.boxes + (size_t)b * a.capacity : nullptr;
    int4 *info = a.info ? a.info + (size_t)b * a.capacity : nullptr;
    int carry_start = -1;  // the last column at or before the chunk that starts a segment
    int carry_kept = 0;    // kept segments that end before the chunk
    for (unsigned base = 0; base < (unsigned)a.Wv; base += STIXEL_THREADS) {  // uniform: every thread reaches the barriers
        const bool inside = base + tid < (unsigned)a.Wv;  // unsigned: Wv may be within 256 of 2^31
        const int i = inside ? (int)(base + tid) : 0;
        bool ends = false;
        int start = -1;
        if (inside) {
            const int4 me = L[i];
            if (me.x >= 0) {
                bool starts = true;
                if (i > 0) {
                    const int4 left = L[i - 1];
                    const int e = me.z - left.z;
                    starts = left.x < 0 || (e < 0 ? -e : e) > a.sim_cols;
                }
                ends = true;
                if (i + 1 < a.Wv) {
                    const int4 right = L[i + 1];
                    const int e = right.z - me.z;
                    ends = right.x < 0 || (e < 0 ? -e : e) > a.sim_cols;
                }
                if (starts) start = i;
            }
        }
        // the running maximum of the start positions: where the segment of column i began
        start = wave_inclusive_max(start);
        if (lane == 63) s_start[wave] = start;
        __syncthreads();
        int before = carry_start, all = carry_start;
        for (int k = 0; k < WAVES; k++) {
            const int w = s_start[k];
            if (k < wave && w > before) before = w;
            if (w > all) all = w;
        }
        if (before > start) start = before;
        const bool kept = ends && i - start + 1 >= a.min_cols;  // ends: column i has a stixel, so a segment began at or before it
        // the prefix sum over "ends a kept segment": the segment's output row
        int total;
        const int local = block_exclusive_scan<STIXEL_THREADS>(kept ? 1 : 0, s_kept, &total);
        if (kept && carry_kept + local < a.capacity) s_first[local] = start, s_last[local] = i;
        __syncthreads();
        // the chunk's segments with an output row, a wavefront each; rows at and beyond the capacity are counted, not written
        int n_out = a.capacity - carry_kept;
        n_out = n_out < 0 ? 0 : n_out < total ? n_out : total;
        if (boxes || info) {
            for (int k = wave; k < n_out; k += WAVES) {
                const int c0 = s_first[k], c1 = s_last[k], n_cols = c1 - c0 + 1;
                int v_top = 0x7FFFFFFF, v_bot = -1, q_lo = 0x7FFFFFFF, q_hi = -1;
                for (unsigned o = lane; o < (unsigned)n_cols; o += 64) {
                    const int4 s = L[c0 + o];
                    v_top = s.y < v_top ? s.y : v_top;
                    v_bot = s.x > v_bot ? s.x : v_bot;
                    q_lo = s.z < q_lo ? s.z : q_lo;
                    q_hi = s.z > q_hi ? s.z : q_hi;
                }
                v_top = wave_min(v_top), v_bot = wave_max(v_bot), q_lo = wave_min(q_lo), q_hi = wave_max(q_hi);
                // the smallest x with #{q_base <= x} >= rank; lo and hi are the same in every lane
                const int rank = (n_cols + 1) / 2;
                int lo = q_lo, hi = q_hi;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    int below = 0;
                    for (unsigned o = lane; o < (unsigned)n_cols; o += 64) below += L[c0 + o].z <= mid ? 1 : 0;
                    below = wave_sum(below);
                    if (below >= rank)
                        hi = mid;
                    else
                        lo = mid + 1;
                }
                if (lane == 0) {
                    const int row = carry_kept + k;  // < capacity
                    // c0 * col_step < W and (c1 - c0) * col_step < W: no overflow
                    if (boxes) boxes[row] = make_int4(c0 * a.col_step, v_top, (c1 - c0) * a.col_step + 1, v_bot - v_top + 1);
                    if (info) info[row] = make_int4(n_cols, q_lo, q_hi, lo);
                }
            }
        }
        carry_start = all;
        carry_kept += total;
        __syncthreads();  // s_start, s_kept, s_first and s_last are rewritten by the next chunk
    }
    if (tid == 0) a.counts[b] = carry_kept;
}

}  // namespace

hipError_t launch_stixel_columns(const StixelArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_stixel_columns, dim3(((unsigned)a.Wv + STIXEL_COLUMNS - 1) / STIXEL_COLUMNS, batch), dim3(STIXEL_COLUMNS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_stixel_objects(const StixelArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_stixel_objects, dim3(batch), dim3(STIXEL_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
