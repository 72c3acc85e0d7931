// Mean 3-D position of the points inside detector boxes, per (box, pair): the step of publishPointCloud (stereo_vision.cpp:261-278)
// that sv_legacy_box_means restates for one frame on the host, here batched and fused with the reprojection (no cloud is written).
// Specified in include/stereo_vision_hip.h (E), restated in stereo_vision/sv.py: box_positions.
//
//   box       columns [clamp(x), clamp(x + w)), rows [clamp(y), clamp(y + h)), clamp(a) = min(max(a, 0), size - 1): the reference's
//             clamp, so the map's last column and row are never part of a box; x + w and y + h in 64 bits
//   pixel     q = the quantised disparity (quarter pixels), P = its point, both from reproject.h's arithmetic
//   select    ALL every pixel / VALID the valid ones / NEAR the valid ones with |q - q_med| <= band, q_med the lower median of q over the
//             box's valid pixels, from a 4096-bin histogram in LDS (integer atomics: exact and order-free)
//   sum       one workgroup per box, a lane per column: the lane adds its column's selected points in ascending row order onto +0.0,
//             then ONE lane per coordinate adds the column sums left to right (every column of the box, 0.0 for one with nothing
//             selected) onto +0.0.  No float atomics, no cross-workgroup combination: the doubles depend on the box and the map alone.
//   pos       sum / (double)n_selected (0 selected: 0.0 / 0.0 = NaN)
//
// Every address is inside the arrays for any box: columns lie in [0, W - 1), rows in [0, H - 1), q in [0, 4095].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "box_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

enum { ADD_NONE = 0, ADD_ALL = 1, ADD_VALID = 2, ADD_NEAR = 3 };

__device__ __forceinline__ int box_clamp(long long v, int size) { return v < 0 ? 0 : (v > size - 1 ? size - 1 : (int)v); }

// One sweep over the box, 256 columns at a time.  HIST: count q of the valid pixels.  ADD: which pixels' points go into the sums;
// lanes 0..2 carry the running totals of X, Y, Z in `acc`.
template <int SRC, int ADD, bool HIST>
__device__ __forceinline__ void box_sweep(const BoxArgs &a, int b, int i_lb, int i_ub, int j_lb, int j_ub, int q_med, uint32_t *hist,
                                          double (*colsum)[256], double &acc) {
    const int tid = threadIdx.x;
    for (int c0 = i_lb; c0 < i_ub; c0 += 256) {
        const int i = c0 + tid;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        if (i < i_ub) {
            for (int j = j_lb; j < j_ub; j++) {
                const size_t n = ((size_t)b * a.H + j) * a.W + i;
                if (SRC == BOX_SRC_POINTS) {
                    const double *p = a.points + 3 * n;
                    sx += p[0], sy += p[1], sz += p[2];
                } else {
                    const float dv = a.disp[n];
                    int q;
                    double d;
                    bool valid;
                    if (SRC == BOX_SRC_DMAP) {
                        q = sv_dmap_u8(dv);
                        d = (double)q;
                        valid = q > 0;
                    } else {
                        valid = dv > 0.f;  // NaN is invalid
                        q = valid ? __float2int_rn(fminf(dv * 4.0f, (float)(BOX_BINS - 1))) : 0;
                        d = (double)dv;
                    }
                    if (HIST && valid) atomicAdd(&hist[q], 1u);
                    bool add = ADD == ADD_ALL;
                    if (ADD == ADD_VALID) add = valid;
                    if (ADD == ADD_NEAR) add = valid && (q > q_med ? q - q_med : q_med - q) <= a.band;
                    if (ADD != ADD_NONE && add) {
                        double X, Y, Z;
                        sv_reproject_point(a.rp, (double)i, (double)j, d, X, Y, Z);
                        sx += X, sy += Y, sz += Z;
                    }
                }
            }
        }
        if (ADD != ADD_NONE) {
            colsum[0][tid] = sx, colsum[1][tid] = sy, colsum[2][tid] = sz;
            __syncthreads();
            if (tid < 3) {
                const int n = i_ub - c0 < 256 ? i_ub - c0 : 256;
                for (int k = 0; k < n; k++) acc += colsum[tid][k];
            }
            __syncthreads();
        }
    }
}

template <int SRC, int SEL>
__global__ __launch_bounds__(256) void k_box_positions(BoxArgs a) {
    __shared__ uint32_t hist[SRC == BOX_SRC_POINTS ? 1 : BOX_BINS];
    __shared__ double colsum[3][256];
    __shared__ int s_wave[4], s_med, s_sel;
    const int m = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    int nb = a.max_boxes;
    if (a.n_boxes) {
        nb = a.n_boxes[b];
        nb = nb < 0 ? 0 : (nb > a.max_boxes ? a.max_boxes : nb);
    }
    if (m >= nb) return;  // the whole workgroup
    const size_t slot = (size_t)b * a.max_boxes + m;
    const int32_t *bx = a.boxes + 4 * slot;
    const long long x = bx[0], y = bx[1], w = bx[2], h = bx[3];
    const int i_lb = box_clamp(x, a.W), i_ub = box_clamp(x + w, a.W), j_lb = box_clamp(y, a.H), j_ub = box_clamp(y + h, a.H);
    const int ncols = i_ub > i_lb ? i_ub - i_lb : 0, nrows = j_ub > j_lb ? j_ub - j_lb : 0;
    const int n_pixels = ncols * nrows;  // < W * H < 2^31
    const int i_end = nrows ? i_ub : i_lb;  // no pixel: no sweep
    double acc = 0.0;
    int n_valid = -1, q_med = -1, n_sel = n_pixels;

    if constexpr (SRC == BOX_SRC_POINTS) {
        box_sweep<SRC, ADD_ALL, false>(a, b, i_lb, i_end, j_lb, j_ub, 0, hist, colsum, acc);
    } else {
        for (int k = tid; k < BOX_BINS; k += 256) hist[k] = 0;
        if (tid == 0) s_med = -1, s_sel = 0;
        __syncthreads();
        box_sweep<SRC, SEL == BOX_SEL_ALL ? ADD_ALL : (SEL == BOX_SEL_VALID ? ADD_VALID : ADD_NONE), true>(a, b, i_lb, i_end, j_lb, j_ub, 0, hist,
                                                                                                        colsum, acc);
        __syncthreads();
        // prefix sums over the bins: a thread owns 16 consecutive bins; inclusive scan inside the wavefront, then across the four
        int own = 0;
        for (int k = 0; k < BOX_BINS / 256; k++) own += (int)hist[tid * (BOX_BINS / 256) + k];
        const int incl = block_exclusive_scan<256>(own, s_wave, &n_valid) + own;
        const int rank = (n_valid + 1) / 2;  // lower median: the smallest q whose cumulative count reaches it
        if (n_valid > 0 && incl - own < rank && rank <= incl) {  // exactly one thread
            int cum = incl - own;
            for (int k = 0; k < BOX_BINS / 256; k++) {
                cum += (int)hist[tid * (BOX_BINS / 256) + k];
                if (cum >= rank) {
                    s_med = tid * (BOX_BINS / 256) + k;
                    break;
                }
            }
        }
        __syncthreads();
        q_med = s_med;
        if (SEL == BOX_SEL_VALID) n_sel = n_valid;
        if (SEL == BOX_SEL_NEAR) {
            int near = 0;
            if (n_valid > 0)
                for (int k = 0; k < BOX_BINS / 256; k++) {
                    const int q = tid * (BOX_BINS / 256) + k;
                    if ((q > q_med ? q - q_med : q_med - q) <= a.band) near += (int)hist[q];
                }
            if (near) atomicAdd(&s_sel, near);
            __syncthreads();
            n_sel = s_sel;
            if (n_sel > 0) box_sweep<SRC, ADD_NEAR, false>(a, b, i_lb, i_end, j_lb, j_ub, q_med, hist, colsum, acc);
        }
    }
    if (tid < 3) a.pos[3 * slot + tid] = acc / (double)n_sel;
    if (tid == 0 && a.stat) {
        int32_t *s = a.stat + 4 * slot;
        s[0] = n_pixels, s[1] = n_valid, s[2] = q_med, s[3] = n_sel;
    }
}

template <int SRC, int SEL>
hipError_t launch1(const BoxArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL((k_box_positions<SRC, SEL>), dim3(a.max_boxes, batch), dim3(256), 0, st, a);
    return hipGetLastError();
}

template <int SRC>
hipError_t launch_sel(int select, const BoxArgs &a, int batch, hipStream_t st) {
    switch (select) {
        case BOX_SEL_ALL: return launch1<SRC, BOX_SEL_ALL>(a, batch, st);
        case BOX_SEL_VALID: return launch1<SRC, BOX_SEL_VALID>(a, batch, st);
        case BOX_SEL_NEAR: return launch1<SRC, BOX_SEL_NEAR>(a, batch, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_box_positions(int src, int select, const BoxArgs &a, int batch, hipStream_t st) {
    switch (src) {
        case BOX_SRC_POINTS: return select == BOX_SEL_ALL ? launch1<BOX_SRC_POINTS, BOX_SEL_ALL>(a, batch, st) : hipErrorInvalidValue;
        case BOX_SRC_DMAP: return launch_sel<BOX_SRC_DMAP>(select, a, batch, st);
        case BOX_SRC_D1: return launch_sel<BOX_SRC_D1>(select, a, batch, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace sv
