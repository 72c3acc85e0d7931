// Wave64 scans, reductions and run combines shared by the kernel files (device code only, after the HIP runtime); the few ladders that
// stay written out in a kernel say so in a comment that names this header.
//
// All of them are for 1-D workgroups of whole wavefronts (lane = threadIdx.x & 63) and exchange registers by shuffles, so EVERY lane of
// the wavefront must reach the call - for block_exclusive_scan every thread of the workgroup, since it holds barriers.  A lane without
// data passes the operation's neutral value, or a key that no live lane has.  Integers only: the results do not depend on the order.
#pragma once

namespace sv {

template <class T>
__device__ __forceinline__ T wave_inclusive_sum(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, 64);
        v += lane >= off ? o : 0;
    }
    return v;
}

template <class T>
__device__ __forceinline__ T wave_inclusive_max(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, 64);
        v = lane >= off && o > v ? o : v;
    }
    return v;
}

// exclusive prefix sum over the workgroup (NT threads): wavefront scans by shuffles, one barrier pair for the wavefront totals in
// cells[NT / 64] (LDS), which may be reused as soon as the call returns
template <int NT, class T, class Cells>
__device__ __forceinline__ T block_exclusive_scan(T val, Cells cells, T *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_sum(val);
    if (lane == 63) cells[wave] = incl;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        const T c = cells[w];
        base += w < wave ? c : 0;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + incl - val;
}

// The CPU emulation of delaunay_gpu.hip (tests/emu_dg_prepare.cpp) plays threadIdx, __syncthreads and __shfl_up: it sees the scans only.
#ifndef DG_HOST_EMULATION

// xor butterfly: every lane ends with the result
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T x, Op op) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = op(x, __shfl_xor(x, off, 64));
    return x;
}
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
    return wave_reduce(x, [](T a, T o) { return a + o; });
}
template <class T>
__device__ __forceinline__ T wave_min(T x) {
    return wave_reduce(x, [](T a, T o) { return o < a ? o : a; });
}
template <class T>
__device__ __forceinline__ T wave_max(T x) {
    return wave_reduce(x, [](T a, T o) { return o > a ? o : a; });
}

// the set bits of `mask` that belong to lanes below the calling one
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// Runs of equal keys in consecutive lanes: one lane of a run (its tail) issues the atomic for all of them.
struct WaveRun {
    bool head, tail;  // the calling lane is the first / the last lane of its run
    int head_lane;    // the run's first lane: the run so far has lane - head_lane + 1 lanes
};
template <class K>
__device__ __forceinline__ WaveRun wave_run(K key) {
    const int lane = __lane_id();
    const K prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
    WaveRun r;
    r.head = lane == 0 || prev != key;
    r.tail = lane == 63 || next != key;
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);  // lanes 0..lane
    r.head_lane = 63 - __clzll((long long)(__ballot(r.head) & upto));           // lane 0 is a head: never zero
    return r;
}

// Inclusive segmented scan over the runs: after it a run's tail holds the run's combined payload.  step(d, take) shuffles the payload
// up by d in every lane and combines what arrived where `take` says that it came from the lane's own run.
template <class Step>
__device__ __forceinline__ void wave_run_scan(const WaveRun &r, Step step) {
    const int lane = __lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) step(d, lane - d >= r.head_lane);
}

#endif  // DG_HOST_EMULATION

}  // namespace sv
