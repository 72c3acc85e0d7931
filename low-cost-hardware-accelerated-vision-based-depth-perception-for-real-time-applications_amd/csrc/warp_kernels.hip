// The previous frame's disparity map warped into the current frame - include/stereo_vision_hip.h (AA), restated in stereo_vision/sv.py
// (disparity_warp).  Doubles in the definition's order in front of the pixel (flow_point.h: the functions of group (Z)), integers behind
// it.  Three kernels over grid (256 consecutive pixels of a frame, frame), lanes along u:
//
//   clear    a lane per pixel: its key = 0; the first workgroup of a frame clears the frame's eight counts.  Nothing is assumed of what
//            the workspace or the counts held.
//   splat    a lane per source pixel i = v0 W + u0 of d_prev.  The pose's twelve doubles sit at one address per frame: scalar loads.  A
//            kept source issues one 64-bit integer atomicMax per covered pixel, (pd << 32) | (0xffffffff - i): the largest pd wins, among
//            equals the smallest i, whatever the order of arrival.  A wavefront's sources are neighbours along u and, under a smooth
//            map, so are their targets: neighbouring 8-byte words.  kept and covered: a ballot and a wavefront sum, added in LDS, one
//            integer atomicAdd per workgroup and word.
//   resolve  a lane per target pixel: the key unpacked into expected and source, with d_cur the label and out; the pixels per label by
//            ballot, added in LDS, one integer atomicAdd per workgroup and word.
//
// bounds     a pixel is read and written only for i < H W; a key is touched only at (x, y) with 0 <= x < W and 0 <= y < H; |tu|, |tv| <=
//            2^20 before they become ints, so tu + dx cannot overflow; counts below B * 8.  covered <= 25 H W < 2^31.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "flow_point.h"
#include "warp_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

__global__ __launch_bounds__(WARP_THREADS) void k_warp_clear(WarpArgs a) {
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const long long hw = (long long)a.H * a.W, i = (long long)blockIdx.x * WARP_THREADS + tid;
    if (i < hw) a.keys[(size_t)b * hw + (size_t)i] = 0ull;
    if (blockIdx.x == 0 && tid < WARP_COUNT_WORDS) a.counts[(size_t)b * WARP_COUNT_WORDS + tid] = 0;
}

__global__ __launch_bounds__(WARP_THREADS) void k_warp_splat(WarpArgs a) {
    __shared__ int s_cnt[2];
    const int tid = (int)threadIdx.x, lane = tid & 63, b = (int)blockIdx.y;
    const long long hw = (long long)a.H * a.W, i = (long long)blockIdx.x * WARP_THREADS + tid;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();

    bool kept = false;
    int covered = 0;
    if (i < hw) {
        const int v0 = (int)(i / a.W), u0 = (int)(i - (long long)v0 * a.W);
        const int d0q = flow_dq(a.d_prev[(size_t)b * hw + (size_t)i]);
        if (d0q > 0) {
            const FlowCamera &c = a.cam;
            double x, y, z;
            flow_point(c, a.poses + (size_t)b * 12, u0, v0, d0q, x, y, z);  // the pose: the same address in every lane
            if (z > FLOW_Z_MIN) {  // false for NaN
                const double pdd = floor(16.0 * (c.fb / z) + 0.5);
                const double fu = floor(((c.f * x) / z + c.cx) + 0.5), fv = floor(((c.f * y) / z + c.cy) + 0.5);
                if (pdd >= 1.0 && pdd <= (double)WARP_PD_MAX && fabs(fu) <= FLOW_CENTRE_MAX && fabs(fv) <= FLOW_CENTRE_MAX) {  // false for NaN
                    kept = true;
                    const int pd = (int)pdd, tu = (int)fu, tv = (int)fv;
                    const int e = min(a.e_max, (pd + d0q - 1) / d0q - 1);
                    const unsigned long long key = ((unsigned long long)pd << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
                    unsigned long long *keys = a.keys + (size_t)b * hw;
                    for (int dy = 0; dy <= e; dy++) {
                        const int ty = tv + dy;
                        if (ty < 0 || ty >= a.H) continue;
                        for (int dx = 0; dx <= e; dx++) {
                            const int tx = tu + dx;
                            if (tx < 0 || tx >= a.W) continue;
                            atomicMax(keys + (size_t)ty * a.W + tx, key);
                            covered++;
                        }
                    }
                }
            }
        }
    }
    const int n_kept = __popcll(__ballot(kept)), n_cov = wave_sum(covered);  // every lane of the workgroup gets here
    if (lane == 0) {
        if (n_kept) atomicAdd(&s_cnt[0], n_kept);
        if (n_cov) atomicAdd(&s_cnt[1], n_cov);
    }
    __syncthreads();
    if (tid < 2 && s_cnt[tid]) atomicAdd(a.counts + (size_t)b * WARP_COUNT_WORDS + tid, s_cnt[tid]);
}

__global__ __launch_bounds__(WARP_THREADS) void k_warp_resolve(WarpArgs a) {
    __shared__ int s_cnt[6];
    const int tid = (int)threadIdx.x, lane = tid & 63, b = (int)blockIdx.y;
    const long long hw = (long long)a.H * a.W, i = (long long)blockIdx.x * WARP_THREADS + tid;
    if (tid < 6) s_cnt[tid] = 0;
    __syncthreads();

    int label = -1;  // a lane behind the frame's last pixel
    if (i < hw) {
        const size_t at = (size_t)b * hw + (size_t)i;
        const unsigned long long key = a.keys[at];
        const int ex = (int)(key >> 32);  // 0: no source reached the pixel
        a.expected[at] = ex;
        a.source[at] = ex > 0 ? (int)(0xffffffffu - (uint32_t)key) : -1;
        if (a.d_cur) {
            const uint32_t bits = reinterpret_cast<const uint32_t *>(a.d_cur)[at];
            const int mq = flow_dq(__uint_as_float(bits));
            const int t = a.tol_q + ((a.rel_q * ex) >> 8);  // rel_q <= 256, ex <= 2^20: below 2^29
            if (mq == 0) label = ex > 0 ? 2 : 0;
            else if (ex == 0) label = 1;
            else if (mq > ex + t) label = 4;
            else if (mq < ex - t) label = 5;
            else label = 3;
            a.label[at] = (uint8_t)label;
            uint32_t o = 0xBF800000u;  // -1.0f
            if (a.mode == WARP_MODE_FILL) {
                if (mq > 0) o = bits;
                else if (ex > 0) o = __float_as_uint((float)ex / 16.0f);  // ex <= 2^20: exact
            } else if (a.mode == WARP_MODE_CONFIRM) {
                if (label == 3) o = bits;
            } else {
                if (label == 1 || label == 3) o = bits;
            }
            reinterpret_cast<uint32_t *>(a.out)[at] = o;
        } else {
            label = ex > 0 ? 2 : 0;
        }
    }
#pragma unroll
    for (int l = 0; l < 6; l++) {
        const int n = __popcll(__ballot(label == l));  // every lane of the workgroup gets here
        if (lane == 0 && n) atomicAdd(&s_cnt[l], n);
    }
    __syncthreads();
    if (tid < 6 && s_cnt[tid]) atomicAdd(a.counts + (size_t)b * WARP_COUNT_WORDS + 2 + tid, s_cnt[tid]);
}

}  // namespace

hipError_t launch_disparity_warp(const WarpArgs &a, hipStream_t st) {
    const long long hw = (long long)a.H * a.W;
    if (a.B < 1 || a.B > 65535 || hw < 1 || hw >= (1ll << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((hw + WARP_THREADS - 1) / WARP_THREADS), (unsigned)a.B);
    hipLaunchKernelGGL(k_warp_clear, grid, dim3(WARP_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    hipLaunchKernelGGL(k_warp_splat, grid, dim3(WARP_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    hipLaunchKernelGGL(k_warp_resolve, grid, dim3(WARP_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
