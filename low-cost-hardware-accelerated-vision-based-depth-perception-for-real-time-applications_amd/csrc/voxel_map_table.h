// The rules that make the world-fixed voxel map one map across its stages - insert and read-out (voxel_map_kernels.hip), match
// (voxel_match_kernels.hip), carry (voxel_carry_kernels.hip), carve (voxel_carve_kernels.hip), render (voxel_render_kernels.hip), flatten
// (voxel_flatten_kernels.hip), clusters (voxel_cluster_kernels.hip), align (voxel_align_kernels.hip), normals and plane sums (voxel_normal_kernels.hip) -, written down once: the buffer's parts, the entry's words, the hash, the two probes, a row's way from the
// frame into a cell, and a voxel's centre and height.  Plain inline functions and named constants; what a stage does with an entry it
// has found stays in the stage.  The layout is voxel_map_kernels.h's; the definitions are include/stereo_vision_hip.h (Q)'s.  The
// per-frame voxel cloud (voxel_kernels.hip) has another entry and another life cycle and shares nothing with this.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"

namespace sv {

constexpr unsigned long long VMAP_EMPTY = ~0ull;  // a key is < 2^60, so the all-ones word is free to mean "no voxel here"

enum {  // the 64-bit words of an entry
    VMAP_KEY = 0,
    VMAP_N = 1,   // total weight
    VMAP_S = 2,   // [3] offset sums
    VMAP_C = 5,   // [4] colour sums
    VMAP_M = 9,   // rows
    VMAP_SEQ = 10  // first_seq (low half), last_seq (high half)
};

constexpr unsigned long long VMAP_SEQ_CLEARED = 0xFFFFFFFFull;  // first_seq all ones, last_seq 0: with zeros in the words between, a slot just claimed

__host__ __device__ inline uint32_t vmap_first_seq(unsigned long long seq) { return (uint32_t)seq; }
__host__ __device__ inline uint32_t vmap_last_seq(unsigned long long seq) { return (uint32_t)(seq >> 32); }

// Where the probe sequence of `key` starts.  log2_slots in 1 .. 32 (a map's: 10 .. 27).
__host__ __device__ inline uint32_t vmap_slot_of(int log2_slots, unsigned long long key) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots));
}

// Frame b's rows, as far as the input holds them; below 1 for a frame without any.
__host__ __device__ inline int vmap_rows_of(const int32_t *counts, int b, int cap) {
    const int cnt = counts[b];
    return cnt < cap ? cnt : cap;
}

// A voxel's key: 20 bits per axis.  The part of cell c on axis k, the key of three cells, and the cell on axis k of a key.
__host__ __device__ inline unsigned long long vmap_key_part(long long c, int k) { return (unsigned long long)c << (20 * k); }
__host__ __device__ inline unsigned long long vmap_key(long long cx, long long cy, long long cz) { return vmap_key_part(cx, 0) | vmap_key_part(cy, 1) | vmap_key_part(cz, 2); }
__host__ __device__ inline int32_t vmap_key_cell(unsigned long long key, int k) { return (int32_t)((key >> (20 * k)) & 0xFFFFFull); }

// The 16-bit offset of t inside its cell c.
__host__ __device__ inline long long vmap_offset(double t, long long c) {
    const long long f = (long long)((t - (double)c) * 65536.0);
    return f > 65535 ? 65535 : f;
}

// A voxel's centre on axis k - the read-out's, which the render shares -: lo + (c + (S + 0.5 n) / (65536 n)) * size in double, as written,
// from the key, the axis' offset sum S and the weight n >= 1.
__host__ __device__ inline double vmap_centre(double lo, double size, unsigned long long key, int k, unsigned long long S, unsigned long long n) {
    const double c = (double)vmap_key_cell(key, k);
    return lo + (c + ((double)(long long)S + 0.5 * (double)(long long)n) / (65536.0 * (double)(long long)n)) * size;
}

// A voxel's mean position on axis k in 1/256 of a cell from lo - what the flatten slices by -: c * 256 + ((S / n) >> 8), integers only, from
// the key, the axis' offset sum S and the weight n >= 1.  S / n <= 65535, so the result stays below 2^28.
__host__ __device__ inline int32_t vmap_zq(unsigned long long key, int k, unsigned long long S, unsigned long long n) {
    return vmap_key_cell(key, k) * 256 + (int32_t)((S / n) >> 8);
}

// The read-out's three filters on the entry e, a word of which is only loaded where the ones before it passed.  Args has min_n, min_rows
// and since.
template <class Args>
__host__ __device__ inline bool vmap_passes(const Args &a, const unsigned long long *e) {
    return (long long)e[VMAP_N] >= a.min_n && (long long)e[VMAP_M] >= a.min_rows && (int32_t)vmap_last_seq(e[VMAP_SEQ]) >= a.since;
}

#ifdef __HIPCC__

// The parts of a map's buffer: uint32 claimed, uint32 overflowed | uint64 dropped | two spare words | the table | the read-out's tiles.
__device__ __forceinline__ uint32_t *vmap_head(uint8_t *map) { return reinterpret_cast<uint32_t *>(map); }
__device__ __forceinline__ const uint32_t *vmap_head(const uint8_t *map) { return reinterpret_cast<const uint32_t *>(map); }
__device__ __forceinline__ unsigned long long *vmap_dropped(uint8_t *map) { return reinterpret_cast<unsigned long long *>(map + 8); }
__device__ __forceinline__ const unsigned long long *vmap_dropped(const uint8_t *map) { return reinterpret_cast<const unsigned long long *>(map + 8); }
__device__ __forceinline__ unsigned long long *vmap_table(uint8_t *map) { return reinterpret_cast<unsigned long long *>(map + VMAP_HEAD_BYTES); }
__device__ __forceinline__ const unsigned long long *vmap_table(const uint8_t *map) { return reinterpret_cast<const unsigned long long *>(map + VMAP_HEAD_BYTES); }
__device__ __forceinline__ int32_t *vmap_tiles(uint8_t *map, int log2_slots) {
    return reinterpret_cast<int32_t *>(map + VMAP_HEAD_BYTES + ((size_t)VMAP_ENTRY_WORDS * 8 << log2_slots));
}

// The sticky overflow flag, in a kernel beside whose lanes others may set it (the insert, the carry's table kernel): a relaxed load at
// agent scope, which is made anew at every call.
__device__ __forceinline__ uint32_t vmap_overflowed_meanwhile(const uint32_t *head) { return __hip_atomic_load(head + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// The same flag behind a kernel boundary, in a kernel that no writer of it runs beside: a plain load.
__device__ __forceinline__ bool vmap_overflowed_before(const uint8_t *map) { return vmap_head(map)[1] != 0u; }

// The value words of a cleared entry; the key stays as it is.
__device__ __forceinline__ void vmap_clear_values(unsigned long long *e) {
#pragma unroll
    for (int k = VMAP_N; k < VMAP_SEQ; k++) e[k] = 0ull;
    e[VMAP_SEQ] = VMAP_SEQ_CLEARED;
}

// The slot of `key`, or -1 where the map holds none: linear probing from vmap_slot_of, around the table's end, ended by the key, by an
// empty key or after `slots` probes.  Plain loads: for a table into which no kernel beside this one writes keys.
__device__ __forceinline__ long long vmap_find(const unsigned long long *table, int log2_slots, unsigned long long key) {
    const uint32_t last = (uint32_t)(((size_t)1 << log2_slots) - 1);
    uint32_t h = vmap_slot_of(log2_slots, key);
    for (uint32_t probe = 0; probe <= last; probe++, h = (h + 1) & last) {
        const unsigned long long k = table[(size_t)h * VMAP_ENTRY_WORDS + VMAP_KEY];
        if (k == key) return (long long)h;
        if (k == VMAP_EMPTY) return -1;
    }
    return -1;  // a full table without the key
}

// vmap_find's sequence by its steps, for a caller that keeps several probes in flight and steps them side by side: whether a probe for
// `key` that saw `seen` in its slot goes on - it ends at the key and at an empty key; the caller counts to `slots` -, and the slot behind h.
__host__ __device__ inline bool vmap_probe_goes_on(unsigned long long seen, unsigned long long key) { return seen != key && seen != VMAP_EMPTY; }
__host__ __device__ inline uint32_t vmap_next_slot(int log2_slots, uint32_t h) { return (h + 1) & (uint32_t)(((size_t)1 << log2_slots) - 1); }

// The entry of `key`, claimed where the map held none: the same probe sequence with a CAS on the key word that moves on at someone
// else's key and never waits.  A lane looks at the overflow flag every sixteenth probe and gives up where it is set - a full table of a
// map that is lost anyway -, and a sequence that ends without an entry sets it: more voxels than the capacity.  NULL then; claimed where
// the CAS turned an empty key into ours.  The insert (voxel_map_kernels.hip: vmap_add) keeps a copy of this loop around its update, see
// there.
__device__ __forceinline__ unsigned long long *vmap_claim(uint32_t *head, unsigned long long *table, int log2_slots, unsigned long long key, bool &claimed) {
    const uint32_t last = (uint32_t)(((size_t)1 << log2_slots) - 1);
    uint32_t h = vmap_slot_of(log2_slots, key);
    claimed = false;
    for (uint32_t probe = 0; probe <= last; probe++, h = (h + 1) & last) {
        if ((probe & 15) == 15 && vmap_overflowed_meanwhile(head)) break;
        unsigned long long *e = table + (size_t)h * VMAP_ENTRY_WORDS;
        const unsigned long long old = atomicCAS(e + VMAP_KEY, VMAP_EMPTY, key);
        if (old != VMAP_EMPTY && old != key) continue;  // someone else's: the next slot
        claimed = old == VMAP_EMPTY;
        return e;
    }
    atomicOr(head + 1, 1u);
    return nullptr;
}

// Row o of an f32 or f64 [.][3] array, widened to double.
template <int DT>
__device__ __forceinline__ void vmap_load_row(const void *xyz, size_t o, double &x, double &y, double &z) {
    if (DT == VMAP_F32) {
        const float *p = static_cast<const float *>(xyz) + 3 * o;
        x = (double)p[0], y = (double)p[1], z = (double)p[2];
    } else {
        const double *p = static_cast<const double *>(xyz) + 3 * o;
        x = p[0], y = p[1], z = p[2];
    }
}

// A row's coordinate on axis k under `pose` (R row-major, then t): every product and sum rounded on its own, in this order (the build
// has -ffp-contract=off).  The insert's transform; the place descriptor (place_kernels.hip) takes its rows through the same function.
__device__ __forceinline__ double vmap_world(const double *pose, int k, double x, double y, double z) {
    const double P = ((pose[3 * k] * x + pose[3 * k + 1] * y) + pose[3 * k + 2] * z) + pose[9 + k];
    return P;
}

// A row's way into the map on axis k: the world coordinate under `pose`, by vmap_world; the kept rule, which NaN and inf never pass, and-ed with `keep` and
// returned; t in cells from lo, by a real division, 0 for a row that is not kept; the cell c, clamped into the box.  A caller walks k =
// 0, 1, 2 and hands each axis the `keep` of the one before, so a row that fails on an axis has t = 0 on the ones behind it.  `keep` goes
// in and out by value: by reference the kernels' code came out different.  Args has the map's lo, hi, size and nc.
template <class Args>
__device__ __forceinline__ bool vmap_cell(const Args &a, const double *pose, int k, double x, double y, double z, bool keep, double &t, long long &c) {
    const double P = vmap_world(pose, k, x, y, z);
    keep = keep && a.lo[k] < P && P < a.hi[k];  // false for NaN
    t = keep ? (P - a.lo[k]) / a.size : 0.0;
    c = (long long)t;
    if (c > a.nc[k] - 1) c = a.nc[k] - 1;
    return keep;
}

#endif  // __HIPCC__

}  // namespace sv
