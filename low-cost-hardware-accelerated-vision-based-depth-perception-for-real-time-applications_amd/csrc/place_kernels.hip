// Place recognition: the polar height descriptor of a frame of rows, and the search of query descriptors among stored ones under every
// rotation - include/stereo_vision_hip.h (AC), restated in stereo_vision/sv.py (place_descriptor, place_match).  Doubles in the
// definition's order in front of the cell - one operation at a time, the build contracts nothing -, integers behind it; the only
// atomics are integer maxima and counts, so no result depends on the schedule.
//
//   clear    the workspace of the descriptor: per frame kept, dropped, 0, 0 and R * S maxima.
//   bin      grid (chunk of PLACE_CHUNK rows, frame): a lane per row - the insert's transform (vmap_world) where there are poses, the kept
//            rule, qx, qy, the ring by a walk over ring_edge2, the sector by a bisection over the half circle the row lies in (the cross
//            products with dir[h] .. dir[h + S/2 - 1] change sign once), the height code -, the chunk's maxima by atomicMax in LDS, the
//            occupied bins flushed by atomicMax to the workspace.  A chunk behind the frame's count does nothing.
//   pack     a workgroup per frame: four maxima per lane to four bytes of desc, the ring counts and the four words.
//   search   grid (group of PLACE_SHARE keys, query), four wavefronts of sixteen keys.  The query goes into LDS with every ring row
//            doubled along the sectors (pitch 2 S / 4 + 1 dwords), so q[r][(c - s) mod S] is the byte S - s + c of the row and a shift is
//            a byte offset.  The tests - both sums, the gap of the sequence numbers, the ring gate - run four lanes per key, before any
//            difference; a ballot makes the candidates a scalar mask.  Then a wavefront per KB = 4 candidates, a lane per shift (two
//            passes for S > 64): per ring row S / 4 + 1 aligned dwords of the query from LDS, brought into place by v_alignbyte_b32 once
//            for the four keys, whose dwords are the same in every lane - a ring row of the keys is loaded across the lanes a row ahead,
//            put into LDS and read back by every lane, sixteen bytes a read -, four bytes per v_sad_u8.  The least (sad << 8) | shift of the wavefront is the pair's result;
//            the wavefront keeps the best pair under the cross-multiplied compare, the workgroup writes the best of its four as a partial.
//   best     a workgroup per query: the best of the partials - the total order (sad / norm, key) -, the counts, the verdict.
//
// bounds     a row is loaded only below min(counts, cap); bins are indexed by ring < R and sector < S; the query's LDS row is read from
//            dword (S - s) / 4 to (S - s) / 4 + S / 4 <= 2 S / 4, inside the pitch; a key's words only for key < K; a partial per (query,
//            group); pair only for key < K.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "place_kernels.h"
#include "voxel_map_table.h"
#include "wave_ops.h"

namespace sv {

namespace {

__global__ __launch_bounds__(PLACE_THREADS) void k_place_clear(PlaceDescArgs a) {
    const size_t n = (size_t)a.B * (PLACE_HEAD + a.R * a.S);
    for (size_t i = (size_t)blockIdx.x * PLACE_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * PLACE_THREADS) a.work[i] = 0u;
}

template <int DT>
__global__ __launch_bounds__(PLACE_THREADS) void k_place_bin(PlaceDescArgs a) {
    __shared__ uint32_t s_bin[PLACE_BINS_MAX];
    __shared__ int s_dir[2 * PLACE_SECTORS_MAX];
    __shared__ int s_edge2[PLACE_RINGS_MAX + 1];
    __shared__ int s_kept;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const int rows = vmap_rows_of(a.counts, b, a.cap);
    const int begin = (int)blockIdx.x * PLACE_CHUNK;
    if (begin >= rows) return;  // the whole workgroup, in front of every barrier
    const int end = rows - begin < PLACE_CHUNK ? rows : begin + PLACE_CHUNK;
    const int bins = a.R * a.S, half = a.S / 2;
    for (int j = tid; j < bins; j += PLACE_THREADS) s_bin[j] = 0u;
    for (int j = tid; j < 2 * a.S; j += PLACE_THREADS) s_dir[j] = a.dirs[j];
    for (int j = tid; j <= a.R; j += PLACE_THREADS) s_edge2[j] = a.edge2[j];
    if (tid == 0) s_kept = 0;
    __syncthreads();

    const double *pose = a.poses ? a.poses + (size_t)b * 12 : nullptr;
    int kept = 0;
    for (int i = begin + tid; i < end; i += PLACE_THREADS) {
        const size_t o = (size_t)b * a.cap + (size_t)i;
        double x, y, z;
        vmap_load_row<DT>(a.xyz, o, x, y, z);
        if (pose) {
            const double wx = vmap_world(pose, 0, x, y, z), wy = vmap_world(pose, 1, x, y, z), wz = vmap_world(pose, 2, x, y, z);
            x = wx, y = wy, z = wz;
        }
        // every compare is false for NaN, and what passes is finite
        bool keep = (a.n ? a.n[o] : 1) >= 1 && fabs(x) < a.r_max && fabs(y) < a.r_max && a.z_lo <= z && z < a.z_hi;
        if (!keep) continue;
        const int qx = (int)floor(x / a.unit), qy = (int)floor(y / a.unit);  // |x / unit| <= 1024
        const long long d2 = (long long)qx * qx + (long long)qy * qy;
        keep = a.r_min2 <= d2 && d2 < (long long)PLACE_Q * PLACE_Q && (qx != 0 || qy != 0);
        if (!keep) continue;
        int ring = 0;
        while (ring + 1 < a.R && s_edge2[ring + 1] <= (int)d2) ring++;
        // dir[0] = (2^14, 0) and dir[S/2] = -dir[0]: cross(dir[0], q) = 2^14 qy.  Above the axis, or on it ahead, the sector is in 0 ..
        // S/2 - 1, else in S/2 .. S - 1; in either half cross(dir[k], q) >= 0 holds up to the sector and fails behind it.
        const int h = (qy > 0 || (qy == 0 && qx > 0)) ? 0 : half;
        int lo = h, hi = h + half - 1;  // cross(dir[lo], q) >= 0 holds
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_dir[2 * mid] * qy - s_dir[2 * mid + 1] * qx >= 0) lo = mid;
            else hi = mid - 1;
        }
        const double hz = floor((z - a.z_lo) / a.z_unit);
        const uint32_t code = 1u + (hz < 254.0 ? (uint32_t)hz : 254u);
        atomicMax(&s_bin[ring * a.S + lo], code);
        kept++;
    }
    kept = wave_sum(kept);
    if ((tid & 63) == 0 && kept) atomicAdd(&s_kept, kept);
    __syncthreads();
    uint32_t *work = a.work + (size_t)b * (PLACE_HEAD + bins);
    for (int j = tid; j < bins; j += PLACE_THREADS)
        if (s_bin[j]) atomicMax(work + PLACE_HEAD + j, s_bin[j]);
    if (tid == 0) {
        atomicAdd(work, (uint32_t)s_kept);
        atomicAdd(work + 1, (uint32_t)(end - begin - s_kept));
    }
}

__global__ __launch_bounds__(PLACE_THREADS) void k_place_pack(PlaceDescArgs a) {
    __shared__ int s_ring[PLACE_RINGS_MAX];
    __shared__ int s_sum, s_occ;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int bins = a.R * a.S;
    const uint32_t *work = a.work + (size_t)b * (PLACE_HEAD + bins);
    if (tid < PLACE_RINGS_MAX) s_ring[tid] = 0;
    if (tid == 0) s_sum = 0, s_occ = 0;
    __syncthreads();
    uint32_t *desc = reinterpret_cast<uint32_t *>(a.desc + (size_t)b * bins);  // S is a multiple of 4: four bins of one ring per dword
    int sum = 0, occ = 0;
    for (int j = tid; j < bins / 4; j += PLACE_THREADS) {
        uint32_t w = 0;
        int mine = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t v = work[PLACE_HEAD + 4 * j + k];
            w |= v << (8 * k);
            sum += (int)v;
            mine += v ? 1 : 0;
        }
        desc[j] = w;
        if (mine) atomicAdd(&s_ring[4 * j / a.S], mine);
        occ += mine;
    }
    sum = wave_sum(sum), occ = wave_sum(occ);
    if ((tid & 63) == 0) atomicAdd(&s_sum, sum), atomicAdd(&s_occ, occ);
    __syncthreads();
    if (tid < a.R) a.ring[(size_t)b * a.R + tid] = (uint8_t)s_ring[tid];
    if (tid == 0) {
        int32_t *w = a.words + (size_t)b * 4;
        w[0] = s_sum, w[1] = s_occ, w[2] = (int32_t)work[0], w[3] = (int32_t)work[1];
    }
}

// A pair's result and what orders it: key < 0 for none.
struct PlaceBest {
    int key, shift, sad, norm;
};

// a before b in the total order (sad / norm, key); one without a key comes last
__device__ __forceinline__ bool place_before(const PlaceBest &p, const PlaceBest &q) {
    if (p.key < 0 || q.key < 0) return p.key >= 0 && q.key < 0;
    const long long l = (long long)p.sad * q.norm, r = (long long)q.sad * p.norm;
    return l < r || (l == r && p.key < q.key);
}

template <int KB>
__global__ __launch_bounds__(PLACE_MATCH_THREADS) void k_place_search(PlaceMatchArgs a) {
    __shared__ uint32_t s_q[PLACE_BINS_MAX / 2 + PLACE_RINGS_MAX];  // R * pitch dwords: R * S <= 4096 bytes doubled, a dword per row more
    __shared__ uint8_t s_qring[PLACE_RINGS_MAX];
    __shared__ int s_part[PLACE_MATCH_THREADS / 64][6];
    __shared__ uint4 s_key[PLACE_MATCH_THREADS / 64][KB][8];  // per wavefront a ring row of its KB keys, 32 dwords each
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int group = (int)blockIdx.x, q = (int)blockIdx.y;
    const int R = a.R, S = a.S, ND = S / 4, pitch = 2 * ND + 1;
    constexpr int NV = (KB + 1) / 2;  // registers that take a ring row of the KB keys from memory, two keys each

    const uint32_t *qd = reinterpret_cast<const uint32_t *>(a.q_desc + (size_t)q * R * S);
    for (int i = tid; i < R * ND; i += PLACE_MATCH_THREADS) {
        const int r = i / ND, j = i - r * ND;
        const uint32_t v = qd[i];
        s_q[r * pitch + j] = v, s_q[r * pitch + ND + j] = v;
        if (j == 0) s_q[r * pitch + 2 * ND] = v;
    }
    if (tid < R) s_qring[tid] = a.q_ring[(size_t)q * R + tid];
    __syncthreads();

    // the tests: four lanes per key, sixteen keys per wavefront
    const int key0 = group * PLACE_SHARE + wave * 16, mine = key0 + (lane >> 2);
    const int q_sum = a.q_words[(size_t)q * 4];
    const long long q_seq = a.q_seq[q];
    const bool valid = mine < a.K;
    bool pre = false;
    int k_sum = 0;
    if (valid) {
        k_sum = a.k_words[(size_t)mine * 4];
        const long long gap = q_seq - (long long)a.k_seq[mine];
        pre = q_sum > 0 && k_sum > 0 && (gap < 0 ? -gap : gap) >= (long long)a.min_gap;
    }
    bool post = pre;
    if (a.ring_gate >= 0) {  // the same for every lane: all of them reach the shuffles
        int d = 0;
        if (pre) {
            const uint8_t *kr = a.k_ring + (size_t)mine * R;
            for (int r = lane & 3; r < R; r += 4) d += abs((int)s_qring[r] - (int)kr[r]);
        }
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        post = pre && d <= a.ring_gate;
    }
    const unsigned long long firsts = 0x1111111111111111ull;
    const unsigned long long m_pre = __ballot(pre) & firsts;
    unsigned long long m = __ballot(post) & firsts;
    const int n_pre = __popcll(m_pre), n_post = __popcll(m);
    if (a.pair && valid && !post && (lane & 3) == 0) {
        int32_t *p = a.pair + ((size_t)q * a.K + (size_t)mine) * 2;
        p[0] = -1, p[1] = 0;
    }

    // the search: a wavefront per KB candidates, a lane per shift
    PlaceBest top = {-1, 0, -1, 0};
    const uint32_t *kd = reinterpret_cast<const uint32_t *>(a.k_desc);
    while (m) {
        int key[KB];
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
            key[kb] = m ? key0 + (__builtin_ctzll(m) >> 2) : -1;
            m &= m - 1;  // 0 stays 0
        }
        const uint32_t *kp[KB];
#pragma unroll
        for (int kb = 0; kb < KB; kb++) kp[kb] = kd + (size_t)(key[kb] < 0 ? key[0] : key[kb]) * R * ND;  // a pass without a key repeats the first
        uint32_t least[KB];
#pragma unroll
        for (int kb = 0; kb < KB; kb++) least[kb] = 0xFFFFFFFFu;
        // A ring row of the keys - ND <= 32 dwords each - is loaded across the lanes, key 2 h in lanes 0 .. 31 of ahead[h], key 2 h + 1 in
        // lanes 32 .. 63, a row ahead of its use, and put into the wavefront's part of LDS, from where every lane reads it back four dwords
        // at a time (one address: a broadcast).  The store waits for a load that has had a row's sums to arrive; the sums wait for LDS
        // only.  Every lane loads and walks the rows - the control flow is the wavefront's -; a lane without a shift reads the query at
        // offset S and drops what it summed.
        const int part = lane & 31, upper = lane >> 5;
        uint32_t *keys = reinterpret_cast<uint32_t *>(s_key[wave]);
        auto load_row = [&](int r, uint32_t *into) {
#pragma unroll
            for (int h = 0; h < NV; h++) {
                const int kb = 2 * h + upper;
                into[h] = kb < KB && part < ND ? kp[kb < KB ? kb : 0][r * ND + part] : 0u;
            }
        };
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane, back = s < S - s ? s : S - s;
            const bool shift = s < S && back <= a.max_shift;
            const int o = shift ? S - s : S;  // 1 .. S
            const uint32_t sh = (uint32_t)o & 3u;
            uint32_t acc[KB], ahead[NV];
#pragma unroll
            for (int kb = 0; kb < KB; kb++) acc[kb] = 0u;
            load_row(0, ahead);
            for (int r = 0; r < R; r++) {
#pragma unroll
                for (int h = 0; h < NV; h++)
                    if (2 * h + upper < KB) keys[(2 * h + upper) * 32 + part] = ahead[h];
                __builtin_amdgcn_wave_barrier();  // the wavefront's stores, then its loads: LDS keeps a wavefront's order
                if (r + 1 < R) load_row(r + 1, ahead);  // on its way while this row is summed
                const uint32_t *row = s_q + r * pitch + (o >> 2);
                uint32_t cur = row[0];
                // four dwords of each key and four of the query on their way before the first is used; FULL: all four are the row's
                auto block = [&](int j, auto full) {
                    constexpr bool FULL = decltype(full)::value;
                    uint4 kv[KB];
#pragma unroll
                    for (int kb = 0; kb < KB; kb++) kv[kb] = s_key[wave][kb][j >> 2];
                    const int last = FULL ? 4 : ND - j;  // 1 .. 3 in the block behind the full ones: the reads stay inside the row
                    const uint32_t n0 = row[j + 1], n1 = row[j + (last > 1 ? 2 : 1)], n2 = row[j + (last > 2 ? 3 : 1)], n3 = row[j + (last > 3 ? 4 : 1)];
                    const uint32_t c0 = __builtin_amdgcn_alignbyte(n0, cur, sh), c1 = __builtin_amdgcn_alignbyte(n1, n0, sh);
                    const uint32_t c2 = __builtin_amdgcn_alignbyte(n2, n1, sh), c3 = __builtin_amdgcn_alignbyte(n3, n2, sh);
#pragma unroll
                    for (int kb = 0; kb < KB; kb++) {
                        acc[kb] = __builtin_amdgcn_sad_u8(kv[kb].x, c0, acc[kb]);
                        if (last > 1) acc[kb] = __builtin_amdgcn_sad_u8(kv[kb].y, c1, acc[kb]);
                        if (last > 2) acc[kb] = __builtin_amdgcn_sad_u8(kv[kb].z, c2, acc[kb]);
                        if (last > 3) acc[kb] = __builtin_amdgcn_sad_u8(kv[kb].w, c3, acc[kb]);
                    }
                    cur = n3;
                };
                int j = 0;
                for (; j + 4 <= ND; j += 4) block(j, std::true_type{});
                if (j < ND) block(j, std::false_type{});
                __builtin_amdgcn_wave_barrier();  // the row has been read before the next one is stored
            }
#pragma unroll
            for (int kb = 0; kb < KB; kb++) {
                const uint32_t word = acc[kb] << 8 | (uint32_t)s;
                least[kb] = shift && word < least[kb] ? word : least[kb];
            }
        }
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
            if (key[kb] < 0) continue;  // the same in every lane
            const uint32_t word = wave_min(least[kb]);  // shift 0 is always admitted: a word below 2^28
            const PlaceBest got = {key[kb], (int)(word & 255u), (int)(word >> 8), q_sum + a.k_words[(size_t)key[kb] * 4]};
            if (a.pair && lane == 0) {
                int32_t *p = a.pair + ((size_t)q * a.K + (size_t)got.key) * 2;
                p[0] = got.sad, p[1] = got.shift;
            }
            if (place_before(got, top)) top = got;
        }
    }
    if (lane == 0) {
        int *p = s_part[wave];
        p[0] = top.key, p[1] = top.shift, p[2] = top.sad, p[3] = top.norm, p[4] = n_pre, p[5] = n_post;
    }
    __syncthreads();
    if (tid == 0) {
        PlaceBest all = {-1, 0, -1, 0};
        int before = 0, behind = 0;
        for (int w = 0; w < PLACE_MATCH_THREADS / 64; w++) {
            const PlaceBest got = {s_part[w][0], s_part[w][1], s_part[w][2], s_part[w][3]};
            if (place_before(got, all)) all = got;
            before += s_part[w][4], behind += s_part[w][5];
        }
        int32_t *p = a.part + ((size_t)q * a.n_groups + (size_t)group) * PLACE_PART_WORDS;
        p[0] = all.key, p[1] = all.shift, p[2] = all.sad, p[3] = all.norm, p[4] = before, p[5] = behind, p[6] = 0, p[7] = 0;
    }
}

__global__ __launch_bounds__(PLACE_THREADS) void k_place_best(PlaceMatchArgs a) {
    __shared__ int s_part[PLACE_THREADS / 64][6];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (int)blockIdx.x;
    PlaceBest top = {-1, 0, -1, 0};
    int before = 0, behind = 0;
    for (int g = tid; g < a.n_groups; g += PLACE_THREADS) {  // no group for K == 0
        const int32_t *p = a.part + ((size_t)q * a.n_groups + (size_t)g) * PLACE_PART_WORDS;
        const PlaceBest got = {p[0], p[1], p[2], p[3]};
        if (place_before(got, top)) top = got;
        before += p[4], behind += p[5];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const PlaceBest got = {__shfl_xor(top.key, off, 64), __shfl_xor(top.shift, off, 64), __shfl_xor(top.sad, off, 64), __shfl_xor(top.norm, off, 64)};
        if (place_before(got, top)) top = got;
    }
    before = wave_sum(before), behind = wave_sum(behind);
    if (lane == 0) {
        int *p = s_part[wave];
        p[0] = top.key, p[1] = top.shift, p[2] = top.sad, p[3] = top.norm, p[4] = before, p[5] = behind;
    }
    __syncthreads();
    if (tid == 0) {
        PlaceBest all = {-1, 0, -1, 0};
        before = 0, behind = 0;
        for (int w = 0; w < PLACE_THREADS / 64; w++) {
            const PlaceBest got = {s_part[w][0], s_part[w][1], s_part[w][2], s_part[w][3]};
            if (place_before(got, all)) all = got;
            before += s_part[w][4], behind += s_part[w][5];
        }
        const bool ok = all.key >= 0 && 256ll * all.sad <= (long long)a.accept * all.norm;
        int32_t *o = a.best + (size_t)q * 4, *c = a.counts + (size_t)q * 3;
        o[0] = ok ? all.key : -1, o[1] = all.shift, o[2] = all.sad, o[3] = all.norm;  // (-1, 0, -1, 0) without a candidate
        c[0] = before, c[1] = behind, c[2] = ok ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_place_descriptor(const PlaceDescArgs &a, hipStream_t st) {
    const size_t n = (size_t)a.B * (PLACE_HEAD + a.R * a.S);
    const unsigned clear = (unsigned)((n + PLACE_THREADS - 1) / PLACE_THREADS < 1024 ? (n + PLACE_THREADS - 1) / PLACE_THREADS : 1024);
    hipLaunchKernelGGL(k_place_clear, dim3(clear), dim3(PLACE_THREADS), 0, st, a);
    if (a.n_chunks > 0) {
        if (a.f64) hipLaunchKernelGGL(k_place_bin<VMAP_F64>, dim3((unsigned)a.n_chunks, (unsigned)a.B), dim3(PLACE_THREADS), 0, st, a);
        else hipLaunchKernelGGL(k_place_bin<VMAP_F32>, dim3((unsigned)a.n_chunks, (unsigned)a.B), dim3(PLACE_THREADS), 0, st, a);
    }
    hipLaunchKernelGGL(k_place_pack, dim3((unsigned)a.B), dim3(PLACE_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_place_match(const PlaceMatchArgs &a, hipStream_t st) {
    if (a.n_groups > 0) {
        const dim3 grid((unsigned)a.n_groups, (unsigned)a.Q);
        if (a.flags & PLACE_ONE_KEY) hipLaunchKernelGGL(k_place_search<1>, grid, dim3(PLACE_MATCH_THREADS), 0, st, a);
        else hipLaunchKernelGGL(k_place_search<4>, grid, dim3(PLACE_MATCH_THREADS), 0, st, a);
    }
    hipLaunchKernelGGL(k_place_best, dim3((unsigned)a.Q), dim3(PLACE_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
