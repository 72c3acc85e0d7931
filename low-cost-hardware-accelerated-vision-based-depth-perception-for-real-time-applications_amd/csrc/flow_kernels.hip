// Stereo visual odometry: the temporal matches of two frames and the sums of one round of the egomotion fit - include/stereo_vision_hip.h
// (Z), restated in stereo_vision/sv.py (flow_match, flow_pose_sums).  Doubles in the definition's order in front of the pixel - one
// operation at a time, the build contracts nothing -, integers behind it.  Four kernels, no atomics, and no workgroup waits for another:
//
//   match    grid (four lattice points, frame): a wavefront per lattice point (u0, v0) = step * (p % nlx, p / nlx).  The point's test,
//            its d0q and the window's centre c are the same in every lane.  The window of cur around c, (2 wx + 2 r + 1) x (2 wy + 2 r + 1)
//            bytes from (c.x - wx - r, c.y - wy - r) on, goes into the wavefront's part of LDS as rows of `pitch` dwords, bytes outside the
//            image as 0 (no candidate that is admitted reads them).  The patch of prev goes into (2 r + 1) * ND lanes, a dword each, the
//            bytes behind the patch's row 0, and from there into scalars by readlane.  Then the lanes go over the candidates, index ci =
//            (dy + wy) (2 wx + 1) + (dx + wx) = lane, lane + 64, ...: per patch row ND + 1 aligned dwords of the window, brought into
//            place by v_alignbyte_b32, the last masked to the patch's width, four bytes per v_sad_u8.  A lane keeps the two least keys
//            (cost << 14 | ci) of its candidates.  The best is the wavefront's least key.  The second - the least cost among the
//            candidates more than one step from the best in dx or dy - needs the best first: a lane answers with its least key if that
//            is far from the best, else with its second least if that is far, and a lane both of whose keys are near the best - two of
//            the best's nine neighbours fall into one lane only where 2 wx + 1 is 1 off a multiple of 32 - walks its candidates again.
//            Lane 0 writes the point's record: d0q = 0 for a point without a match.
//   pack     a workgroup per frame: the records with d0q > 0 in point order - flag, workgroup scan, rank, tile by tile - into matches
//            and cost up to the capacity, -1 into the rows behind them, the count (or -1) into counts.
//   score    grid (chunk of 256 matches, frame): a lane per match, its 32 words in registers, wave_sum, the four wavefronts' words added
//            in LDS and stored as the chunk's partial - zeros for a chunk behind the frame's count.
//   sums     a workgroup per frame adds the partials.
//
// bounds     a lattice point is loaded only for p < nlx * nly and r <= u0 < W - r, r <= v0 < H - r; a byte of cur only inside the image; the
//            window's dwords are indexed below pitch * rows <= 4096 per wavefront; a record below nlx * nly; a match below min(count,
//            capacity); d_cur at (u1, v1), a candidate that was admitted and lies inside the image.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "flow_kernels.h"
#include "flow_point.h"
#include "wave_ops.h"

namespace sv {

namespace {

constexpr uint32_t FLOW_NONE = 0xFFFFFFFFu;
constexpr double FLOW_PIXEL_MAX = 1073741824.0;  // flow_point.h: flow_dq, flow_point, FLOW_Z_MIN, FLOW_CENTRE_MAX

template <int R>
struct Patch {
    static constexpr int SIDE = 2 * R + 1, ND = (SIDE + 3) / 4, WORDS = SIDE * ND;
    static constexpr uint32_t LAST = 0xFFFFFFFFu >> (8 * (4 * ND - SIDE));  // the bytes of a row's last dword that belong to the patch
    uint32_t w[WORDS];
};

// the sum of absolute differences of the patch and the window's (2 R + 1)^2 bytes from byte ox of row oy on
template <int R>
__device__ __forceinline__ uint32_t flow_cost(const Patch<R> &pp, const uint32_t *win, int pitch, int ox, int oy) {
    constexpr int ND = Patch<R>::ND;
    const uint32_t *row = win + oy * pitch + (ox >> 2);
    const uint32_t sh = (uint32_t)ox & 3u;
    uint32_t acc = 0;
#pragma unroll
    for (int py = 0; py < Patch<R>::SIDE; py++, row += pitch) {
        uint32_t in[ND + 1];
#pragma unroll
        for (int j = 0; j <= ND; j++) in[j] = row[j];
#pragma unroll
        for (int j = 0; j < ND; j++) {
            uint32_t c = __builtin_amdgcn_alignbyte(in[j + 1], in[j], sh);
            if (j == ND - 1) c &= Patch<R>::LAST;
            acc = __builtin_amdgcn_sad_u8(pp.w[py * ND + j], c, acc);
        }
    }
    return acc;
}

template <int R>
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_match(FlowMatchArgs a) {
    extern __shared__ uint32_t s_win[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)blockIdx.y;
    const long long nl = (long long)a.nlx * a.nly;
    const long long p = (long long)blockIdx.x * FLOW_WAVES + wave;
    uint32_t *win = s_win + (size_t)wave * a.pitch * a.rows;
    const size_t frame = (size_t)b * a.H * a.W;
    const int nwx = 2 * a.wx + 1, ncand = nwx * (2 * a.wy + 1);

    // the point: the same in every lane
    bool live = p < nl;
    int u0 = 0, v0 = 0, d0q = 0, ccx = 0, ccy = 0;
    if (live) {
        u0 = (int)(p % a.nlx) * a.step, v0 = (int)(p / a.nlx) * a.step;
        live = u0 >= R && u0 < a.W - R && v0 >= R && v0 < a.H - R;
    }
    if (live) {
        d0q = flow_dq(a.d_prev[frame + (size_t)v0 * a.W + u0]);
        live = d0q > 0;
    }
    ccx = u0, ccy = v0;
    if (live && a.guess) {
        double x, y, z;
        flow_point(a.cam, a.guess + (size_t)b * 12, u0, v0, d0q, x, y, z);
        live = z > FLOW_Z_MIN;  // false for NaN
        if (live) {
            const double fx = floor(((a.cam.f * x) / z + a.cam.cx) + 0.5), fy = floor(((a.cam.f * y) / z + a.cam.cy) + 0.5);
            live = fabs(fx) <= FLOW_CENTRE_MAX && fabs(fy) <= FLOW_CENTRE_MAX;  // false for NaN
            if (live) ccx = (int)fx, ccy = (int)fy;
        }
    }
    if (live) {  // a candidate at all?
        const int x_lo = max(ccx - a.wx, R), x_hi = min(ccx + a.wx, a.W - R - 1), y_lo = max(ccy - a.wy, R), y_hi = min(ccy + a.wy, a.H - R - 1);
        live = x_lo <= x_hi && y_lo <= y_hi;
    }
    Patch<R> pp;
    if (live) {
        const int gx0 = ccx - a.wx - R, gy0 = ccy - a.wy - R;
        const uint8_t *cur = a.cur + frame;
        for (int i = lane; i < a.pitch * a.rows; i += 64) {
            const int row = i / a.pitch, gy = gy0 + row, gx = gx0 + 4 * (i - row * a.pitch);
            uint32_t v = 0;
            if (gy >= 0 && gy < a.H) {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (gx + k >= 0 && gx + k < a.W) v |= (uint32_t)cur[(size_t)gy * a.W + gx + k] << (8 * k);
            }
            win[i] = v;
        }
        uint32_t mine = 0;
        if (lane < Patch<R>::WORDS) {
            const int row = lane / Patch<R>::ND, col = 4 * (lane % Patch<R>::ND);
            const uint8_t *src = a.prev + frame + (size_t)(v0 - R + row) * a.W + (u0 - R);
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (col + k < Patch<R>::SIDE) mine |= (uint32_t)src[col + k] << (8 * k);
        }
#pragma unroll
        for (int i = 0; i < Patch<R>::WORDS; i++) pp.w[i] = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
    }
    __syncthreads();  // every thread of the workgroup gets here: the windows are written

    uint32_t best = FLOW_NONE, second = FLOW_NONE;
    int box = 0, boy = 0;
    if (live) {
        const int tx0 = ccx - a.wx, ty0 = ccy - a.wy;
        uint32_t k1 = FLOW_NONE, k2 = FLOW_NONE;
        for (int ci = lane; ci < ncand; ci += 64) {
            const int oy = ci / nwx, ox = ci - oy * nwx;
            const int tx = tx0 + ox, ty = ty0 + oy;
            if (tx < R || tx >= a.W - R || ty < R || ty >= a.H - R) continue;  // the patch would leave the image
            const uint32_t key = flow_cost<R>(pp, win, a.pitch, ox, oy) << 14 | (uint32_t)ci;
            if (key < k1) k2 = k1, k1 = key;
            else if (key < k2) k2 = key;
        }
        const uint32_t kb = wave_min(k1);  // the least cost, among equals the least index
        if (kb != FLOW_NONE) {
            best = kb >> 14;
            const int bci = (int)(kb & 16383u);
            boy = bci / nwx, box = bci - boy * nwx;
            auto near = [&](uint32_t key) {
                const int ci = (int)(key & 16383u), oy = ci / nwx, ox = ci - oy * nwx;
                return abs(ox - box) <= 1 && abs(oy - boy) <= 1;
            };
            uint32_t sec = FLOW_NONE;
            if (k1 != FLOW_NONE) {
                if (!near(k1)) sec = k1 >> 14;
                else if (k2 == FLOW_NONE) sec = FLOW_NONE;  // the lane's one candidate
                else if (!near(k2)) sec = k2 >> 14;
                else {  // both near the best: the lane's candidates once more, without the best's neighbours
                    for (int ci = lane; ci < ncand; ci += 64) {
                        const int oy = ci / nwx, ox = ci - oy * nwx;
                        const int tx = tx0 + ox, ty = ty0 + oy;
                        if (tx < R || tx >= a.W - R || ty < R || ty >= a.H - R) continue;
                        if (abs(ox - box) <= 1 && abs(oy - boy) <= 1) continue;
                        const uint32_t c = flow_cost<R>(pp, win, a.pitch, ox, oy);
                        sec = c < sec ? c : sec;
                    }
                }
            }
            second = wave_min(sec);
        }
    }
    if (lane == 0 && p < nl) {
        bool ok = live && best != FLOW_NONE && second != FLOW_NONE;
        ok = ok && 256u * best < (uint32_t)a.ratio * second && best <= (uint32_t)a.max_cost;
        const int bdx = box - a.wx, bdy = boy - a.wy;
        ok = ok && !(a.wx > 0 && abs(bdx) == a.wx) && !(a.wy > 0 && abs(bdy) == a.wy);
        int32_t *rec = a.rec + ((size_t)b * nl + (size_t)p) * FLOW_REC_WORDS;
        if (ok) {
            const int u1 = ccx + bdx, v1 = ccy + bdy;  // an admitted candidate: inside the image
            int d1q = -1;
            if (a.d_cur) {
                const int q = flow_dq(a.d_cur[frame + (size_t)v1 * a.W + u1]);
                d1q = q > 0 ? q : -1;
            }
            rec[0] = u0, rec[1] = v0, rec[2] = d0q, rec[3] = u1, rec[4] = v1, rec[5] = d1q, rec[6] = (int)best, rec[7] = (int)second;
        } else {
            rec[2] = 0;
        }
    }
}

__global__ __launch_bounds__(FLOW_THREADS) void k_flow_pack(FlowMatchArgs a) {
    __shared__ int s_cells[FLOW_WAVES];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const long long nl = (long long)a.nlx * a.nly;
    const int32_t *rec = a.rec + (size_t)b * nl * FLOW_REC_WORDS;
    int32_t *m = a.matches + (size_t)b * a.capacity * 6, *c = a.cost + (size_t)b * a.capacity * 2;
    long long base = 0;
    for (long long t0 = 0; t0 < nl; t0 += FLOW_THREADS) {  // the same trips for every thread
        const long long i = t0 + tid;
        const int32_t *r = rec + (size_t)i * FLOW_REC_WORDS;
        const int ok = i < nl && r[2] > 0 ? 1 : 0;
        int total;
        const long long at = base + block_exclusive_scan<FLOW_THREADS>(ok, s_cells, &total);
        if (ok && at < a.capacity) {
#pragma unroll
            for (int k = 0; k < 6; k++) m[at * 6 + k] = r[k];
            c[at * 2] = r[6], c[at * 2 + 1] = r[7];
        }
        base += total;
    }
    for (long long i = (base < a.capacity ? base : a.capacity) + tid; i < a.capacity; i += FLOW_THREADS) {
#pragma unroll
        for (int k = 0; k < 6; k++) m[i * 6 + k] = -1;
        c[i * 2] = -1, c[i * 2 + 1] = -1;
    }
    if (tid == 0) a.counts[b] = base > a.capacity ? -1 : (int)base;
}

// clamp(floor(16 J + 0.5), +-2^20) of a finite J
__device__ __forceinline__ long long flow_jq(double J) {
    const double v = floor(16.0 * J + 0.5), lim = (double)FLOW_J_MAX;
    return (long long)(v < -lim ? -lim : v > lim ? lim : v);
}

__global__ __launch_bounds__(FLOW_SUM_THREADS) void k_flow_score(FlowSumsArgs a) {
    __shared__ unsigned long long s_acc[FLOW_SUM_THREADS / 64][FLOW_SUM_WORDS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (int)blockIdx.x, b = (int)blockIdx.y;
    const int cnt = a.counts[b];
    const int rows = cnt < 0 ? 0 : cnt < a.cap ? cnt : a.cap;
    const int i = chunk * FLOW_SUM_THREADS + tid;
    unsigned long long acc[FLOW_SUM_WORDS];
#pragma unroll
    for (int j = 0; j < FLOW_SUM_WORDS; j++) acc[j] = 0ull;
    if (i < rows) {
        const int32_t *m = a.matches + ((size_t)b * a.cap + (size_t)i) * 6;
        const int u0 = m[0], v0 = m[1], d0 = m[2];
        const long long u1 = m[3], v1 = m[4], d1 = m[5];
        if (d0 >= 1 && d0 <= FLOW_DQ_MAX) {
            const FlowCamera &c = a.cam;
            double x, y, z;
            flow_point(c, a.poses + (size_t)b * 12, u0, v0, d0, x, y, z);  // the pose: the same address in every lane
            if (z > FLOW_Z_MIN) {  // false for NaN
                const double fz = c.f / z, xz = x / z, yz = y / z, bz = c.fb / z;
                const double pu = floor(16.0 * (c.f * xz + c.cx) + 0.5), pv = floor(16.0 * (c.f * yz + c.cy) + 0.5), pd = floor(16.0 * bz + 0.5);
                if (fabs(pu) <= FLOW_PIXEL_MAX && fabs(pv) <= FLOW_PIXEL_MAX && fabs(pd) <= FLOW_PIXEL_MAX) {  // false for NaN
                    acc[0] = 1ull;
                    const long long ru = 16 * u1 - (long long)pu, rv = 16 * v1 - (long long)pv, rd = d1 - (long long)pd;
                    const long long g = a.gate_q;
                    if (ru >= -g && ru <= g && rv >= -g && rv <= g && ru * ru + rv * rv <= g * g) {
                        const bool din = d1 > 0 && rd >= -a.dgate_q && rd <= a.dgate_q;
                        const double aa = fz * xz, cc = fz * yz, ee = bz / z;
                        const long long Ju[6] = {flow_jq(fz), 0, flow_jq(-aa), flow_jq(-(aa * y)), flow_jq(c.f * (1.0 + xz * xz)), flow_jq(-(c.f * yz))};
                        const long long Jv[6] = {0, flow_jq(fz), flow_jq(-cc), flow_jq(-(c.f * (1.0 + yz * yz))), flow_jq(aa * y), flow_jq(c.f * xz)};
                        const long long Jd[6] = {0, 0, din ? flow_jq(-ee) : 0, din ? flow_jq(-(ee * y)) : 0, din ? flow_jq(ee * x) : 0, 0};
                        const long long sd = din ? rd : 0;
                        acc[1] = 1ull, acc[2] = din ? 1ull : 0ull;
                        acc[3] = (unsigned long long)(ru * ru + rv * rv), acc[4] = (unsigned long long)(sd * sd);
                        int at = 11;
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            acc[5 + p] = (unsigned long long)(Ju[p] * ru + Jv[p] * rv + Jd[p] * sd);
#pragma unroll
                            for (int q = p; q < 6; q++) acc[at++] = (unsigned long long)(Ju[p] * Ju[q] + Jv[p] * Jv[q] + Jd[p] * Jd[q]);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < FLOW_SUM_WORDS; j++) {
        const unsigned long long v = wave_sum(acc[j]);  // every lane of the workgroup gets here
        if (lane == 0) s_acc[wave][j] = v;
    }
    __syncthreads();
    if (tid < FLOW_SUM_WORDS) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < FLOW_SUM_THREADS / 64; w++) v += s_acc[w][tid];
        a.partials[((size_t)b * a.n_chunks + (size_t)chunk) * FLOW_SUM_WORDS + tid] = v;
    }
}

__global__ __launch_bounds__(FLOW_SUM_THREADS) void k_flow_sums(FlowSumsArgs a) {
    __shared__ unsigned long long s_part[FLOW_SUM_THREADS / FLOW_SUM_WORDS][FLOW_SUM_WORDS];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int group = tid / FLOW_SUM_WORDS, word = tid % FLOW_SUM_WORDS;  // eight groups of 32 threads, a thread per word
    const unsigned long long *in = a.partials + (size_t)b * a.n_chunks * FLOW_SUM_WORDS + word;
    unsigned long long v = 0;
    for (int c = group; c < a.n_chunks; c += FLOW_SUM_THREADS / FLOW_SUM_WORDS) v += in[(size_t)c * FLOW_SUM_WORDS];
    s_part[group][word] = v;
    __syncthreads();
    if (tid < FLOW_SUM_WORDS) {
        unsigned long long t = 0;
#pragma unroll
        for (int g = 0; g < FLOW_SUM_THREADS / FLOW_SUM_WORDS; g++) t += s_part[g][tid];
        a.sums[(size_t)b * FLOW_SUM_WORDS + tid] = (long long)t;
    }
}

template <int R>
void launch_match(const FlowMatchArgs &a, dim3 grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((k_flow_match<R>), grid, dim3(FLOW_THREADS), lds, st, a);
}

}  // namespace

hipError_t launch_flow_match(const FlowMatchArgs &a, hipStream_t st) {
    const long long nl = (long long)a.nlx * a.nly;
    const size_t lds = (size_t)FLOW_WAVES * 4 * a.pitch * a.rows;
    if (a.r < 1 || a.r > FLOW_R_MAX || lds > (size_t)FLOW_WAVES * FLOW_WINDOW_BYTES || nl < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nl + FLOW_WAVES - 1) / FLOW_WAVES), (unsigned)a.B);
    switch (a.r) {
    case 1: launch_match<1>(a, grid, lds, st); break;
    case 2: launch_match<2>(a, grid, lds, st); break;
    case 3: launch_match<3>(a, grid, lds, st); break;
    case 4: launch_match<4>(a, grid, lds, st); break;
    case 5: launch_match<5>(a, grid, lds, st); break;
    case 6: launch_match<6>(a, grid, lds, st); break;
    default: launch_match<7>(a, grid, lds, st); break;
    }
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    hipLaunchKernelGGL(k_flow_pack, dim3((unsigned)a.B), dim3(FLOW_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_flow_sums(const FlowSumsArgs &a, hipStream_t st) {
    if (a.n_chunks > 0) {
        hipLaunchKernelGGL(k_flow_score, dim3((unsigned)a.n_chunks, (unsigned)a.B), dim3(FLOW_SUM_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    hipLaunchKernelGGL(k_flow_sums, dim3((unsigned)a.B), dim3(FLOW_SUM_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
