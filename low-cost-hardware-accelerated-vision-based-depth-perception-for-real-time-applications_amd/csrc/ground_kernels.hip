// Ground plane, obstacle labels and free space from disparity maps, for a batch: Labayrade's v-disparity line fit in integers and a
// per-column walk.  Specified in include/stereo_vision_hip.h (G), restated in stereo_vision/sv.py (v_disparity, ground_line,
// ground_labels, free_space).
//
//   bin       valid iff d > 0; q = min(rintf(4.0f * d), n_bins - 1): the only floating-point operations of this file, both exact
//   hist      k_ground_hist: a workgroup per (pair, strip of GROUND_STRIP rows), one row at a time in LDS.  A filtered disparity row is
//             long runs of one bin, and LDS atomics on one address serialise, so each wavefront adds a run of equal bins (consecutive
//             lanes = consecutive pixels) with ONE atomic by its first lane, the run length from a ballot of the run heads.  The row is
//             stored (vdisp) and scanned in place; its exclusive prefix sums, n_bins + 1 words, go to the workspace.
//   search    k_ground_search: a workgroup per (pair, horizon row vh), a thread per bottom-row bin qb.  S(vh, qb) is one box per row,
//             two loads from the prefix sums; neighbouring qb read neighbouring words.  The line ql(v) advances by a quotient and a
//             remainder per row - no division in the loop.  Candidates are ranked by the key (S << 32) | ~index with max: the largest
//             S, then the smallest candidate index (vh-major), whatever the order of evaluation.
//   pick      k_ground_pick: a workgroup per pair reduces the keys of its horizon rows and the row totals into ground[b].
//   label     k_ground_label: a lane per column walks from the bottom row upwards - a row of 64 neighbouring columns per load -, with
//             the line's bin for the row in a register (the same quotient / remainder, backwards), the length of the obstacle run in
//             another; it stores the label bytes and ends with the column's free_row / free_disp.
//
// Every load and store is guarded by u < W, v < H, bin < n_bins (+ 1 for the prefix rows) or a candidate index < n_vh / n_qb; every
// word of the workspace that is read was written by an earlier kernel of the same call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ground_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

// The bin of a valid disparity (d > 0; +inf lands in the last bin).
__device__ __forceinline__ int ground_bin(float d, int n_bins) { return (int)fminf(rintf(4.0f * d), (float)(n_bins - 1)); }

template <bool AGGREGATE>
__global__ __launch_bounds__(GROUND_THREADS) void k_ground_hist(GroundArgs a) {
    __shared__ uint32_t s_bins[GROUND_BINS_MAX];
    __shared__ uint32_t s_wave[GROUND_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
    const int per = (a.n_bins + GROUND_THREADS - 1) / GROUND_THREADS;  // <= 16: the thread's run of bins in the scan
    const int lo = tid * per < a.n_bins ? tid * per : a.n_bins, hi = lo + per < a.n_bins ? lo + per : a.n_bins;
    for (int j = tid; j < a.n_bins; j += GROUND_THREADS) s_bins[j] = 0u;
    __syncthreads();
    const int v_end = ((int)blockIdx.x + 1) * GROUND_STRIP < a.H ? ((int)blockIdx.x + 1) * GROUND_STRIP : a.H;
    for (int v = (int)blockIdx.x * GROUND_STRIP; v < v_end; v++) {
        const size_t r = (size_t)b * a.H + v;
        const float *row = a.disp + r * a.W;
        for (int base = 0; base < a.W; base += GROUND_THREADS) {  // uniform: every lane takes part in the ballot
            const int u = base + tid;
            int key = -1;
            if (u < a.W) {
                const float d = row[u];
                if (d > 0.f) key = ground_bin(d, a.n_bins);
            }
            if (AGGREGATE) {
                // issues from the run's head, not from its tail as wave_ops.h's wave_run would: no __shfl_down, and not timed otherwise
                const int prev = __shfl_up(key, 1);
                const bool head = lane == 0 || key != prev;
                const unsigned long long heads = __ballot(head);
                const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
                const int next = above ? lane + 1 + __builtin_ctzll(above) : 64;  // the next run's first lane
                if (head && key >= 0) atomicAdd(&s_bins[key], (uint32_t)(next - lane));
            } else {
                if (key >= 0) atomicAdd(&s_bins[key], 1u);
            }
        }
        __syncthreads();
        if (a.vdisp)
            for (int j = tid; j < a.n_bins; j += GROUND_THREADS) a.vdisp[r * a.n_bins + j] = s_bins[j];
        uint32_t own = 0u;
        for (int j = lo; j < hi; j++) own += s_bins[j];
        uint32_t total;
        uint32_t run = block_exclusive_scan<GROUND_THREADS>(own, s_wave, &total);
        for (int j = lo; j < hi; j++) {
            const uint32_t c = s_bins[j];
            s_bins[j] = run;
            run += c;
        }
        __syncthreads();
        uint32_t *p = a.prefix + r * (a.n_bins + 1);
        for (int j = tid; j < a.n_bins; j += GROUND_THREADS) {
            p[j] = s_bins[j];
            s_bins[j] = 0u;  // for the next row, by the thread that read it
        }
        if (tid == 0) p[a.n_bins] = total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(GROUND_THREADS) void k_ground_search(GroundArgs a) {
    __shared__ unsigned long long s_key[GROUND_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.y, ivh = blockIdx.x;
    const int vh = a.vh_lo + ivh * a.vh_step;  // <= H - 2
    const int den = a.H - 1 - vh;              // >= 1
    const int v0 = vh + 1 > 0 ? vh + 1 : 0;
    const int stride = a.n_bins + 1;
    const uint32_t two_den = 2u * (uint32_t)den;
    const uint32_t *rows = a.prefix + ((size_t)b * a.H + v0) * stride;
    unsigned long long best = 0ull;  // below every key: a key's low word is >= 1
    for (int iq = tid; iq < a.n_qb; iq += GROUND_THREADS) {
        const int qb = (iq + 1) * a.qb_step;                           // < n_bins
        const uint32_t step_q = (uint32_t)qb / (uint32_t)den;          // 2 qb = step_q * 2 den + step_r
        const uint32_t step_r = 2u * ((uint32_t)qb - step_q * (uint32_t)den);
        const uint32_t n0 = 2u * (uint32_t)qb * (uint32_t)(v0 - vh) + (uint32_t)den;  // < 2^31 (heights <= 32768, vh >= -32768)
        int q = (int)(n0 / two_den);
        uint32_t rem = n0 - (uint32_t)q * two_den;
        const uint32_t *p = rows;
        uint32_t S = 0u;
        for (int v = v0; v < a.H; v++) {  // q = ql(v) <= qb
            const int lo = q - a.tol > 0 ? q - a.tol : 0;
            const int hi = q + a.tol + 1 < a.n_bins ? q + a.tol + 1 : a.n_bins;
            S += p[hi] - p[lo];
            p += stride;
            q += (int)step_q;
            rem += step_r;
            if (rem >= two_den) rem -= two_den, q++;
        }
        const uint32_t index = (uint32_t)ivh * (uint32_t)a.n_qb + (uint32_t)iq;  // < 2^16 * 2^12
        const unsigned long long key = ((unsigned long long)S << 32) | (0xFFFFFFFFu - index);
        best = key > best ? key : best;
    }
    best = wave_max(best);
    if ((tid & 63) == 0) s_key[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < GROUND_THREADS / 64; k++) best = s_key[k] > best ? s_key[k] : best;
        a.keys[(size_t)b * a.n_vh + ivh] = best;
    }
}

__global__ __launch_bounds__(GROUND_THREADS) void k_ground_pick(GroundArgs a) {
    __shared__ unsigned long long s_key[GROUND_THREADS / 64];
    __shared__ int s_valid[GROUND_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    unsigned long long best = 0ull;
    for (int i = tid; i < a.n_vh; i += GROUND_THREADS) {
        const unsigned long long k = a.keys[(size_t)b * a.n_vh + i];
        best = k > best ? k : best;
    }
    int valid = 0;  // <= W * H < 2^31
    for (int v = tid; v < a.H; v += GROUND_THREADS) valid += (int)a.prefix[((size_t)b * a.H + v) * (a.n_bins + 1) + a.n_bins];
    best = wave_max(best);
    valid = wave_sum(valid);
    if ((tid & 63) == 0) s_key[tid >> 6] = best, s_valid[tid >> 6] = valid;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < GROUND_THREADS / 64; k++) {
            best = s_key[k] > best ? s_key[k] : best;
            valid += s_valid[k];
        }
        const int S = (int)(best >> 32);
        const uint32_t index = 0xFFFFFFFFu - (uint32_t)best;
        const int ivh = (int)(index / (uint32_t)a.n_qb), iq = (int)(index % (uint32_t)a.n_qb);
        const bool found = S >= a.min_support;
        int32_t *g = a.ground + 4 * (size_t)b;
        g[0] = found ? a.vh_lo + ivh * a.vh_step : -1;
        g[1] = found ? (iq + 1) * a.qb_step : -1;
        g[2] = S;
        g[3] = valid;
    }
}

__global__ __launch_bounds__(GROUND_COLUMNS) void k_ground_label(GroundArgs a) {
    const int b = blockIdx.y, u = (int)blockIdx.x * GROUND_COLUMNS + (int)threadIdx.x;
    if (u >= a.W) return;
    const int32_t *g = a.ground + 4 * (size_t)b;
    const bool none = g[1] < 0;  // "no ground": every valid pixel is below it
    const int vh = none ? -1 : g[0], qb = none ? 0 : g[1];
    const int den = a.H - 1 - vh, two_den = 2 * den;  // den >= 1
    const int step_q = qb / den, step_r = 2 * (qb - step_q * den);
    int gq = qb, rem = den;  // ql(H - 1) = qb: 2 qb den + den = qb * 2 den + den
    const float *col = a.disp + (size_t)b * a.H * a.W + u;
    uint8_t *lab = a.labels ? a.labels + (size_t)b * a.H * a.W + u : nullptr;
    int run = 0, run_row = -1, free_row = -1;
    float run_disp = 0.f, free_disp = 0.f;
    for (int v = a.H - 1; v >= 0; v--) {
        const float d = col[(size_t)v * a.W];
        int label = 0;
        if (d > 0.f) {
            const int e = ground_bin(d, a.n_bins) - (v > vh ? gq : 0);
            label = none ? 3 : e > a.g_tol ? 2 : e < -a.g_tol ? 3 : 1;
        }
        if (lab) lab[(size_t)v * a.W] = (uint8_t)label;
        if (label == 2) {
            if (run == 0) run_row = v, run_disp = d;
            if (++run == a.min_run && free_row < 0) free_row = run_row, free_disp = run_disp;
        } else {
            run = 0;
        }
        if (!lab && free_row >= 0) break;  // nothing above is asked for
        gq -= step_q;  // ql(v - 1): 2 qb less in the numerator
        rem -= step_r;
        if (rem < 0) rem += two_den, gq--;
    }
    if (a.free_row) a.free_row[(size_t)b * a.W + u] = free_row;
    if (a.free_disp) a.free_disp[(size_t)b * a.W + u] = free_disp;
}

}  // namespace

hipError_t launch_ground_hist(const GroundArgs &a, int batch, bool aggregate, hipStream_t st) {
    const dim3 grid((a.H + GROUND_STRIP - 1) / GROUND_STRIP, batch);
    if (aggregate)
        hipLaunchKernelGGL(k_ground_hist<true>, grid, dim3(GROUND_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(k_ground_hist<false>, grid, dim3(GROUND_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ground_search(const GroundArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_ground_search, dim3(a.n_vh, batch), dim3(GROUND_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ground_pick(const GroundArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_ground_pick, dim3(batch), dim3(GROUND_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ground_label(const GroundArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_ground_label, dim3((a.W + GROUND_COLUMNS - 1) / GROUND_COLUMNS, batch), dim3(GROUND_COLUMNS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
