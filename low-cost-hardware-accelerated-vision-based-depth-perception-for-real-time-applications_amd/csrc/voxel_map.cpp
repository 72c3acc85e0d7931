// Group (Q) of include/stereo_vision_hip.h: a world-fixed voxel map fed with per-frame clouds along poses (voxel_map_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_map_kernels.h"
#include "voxel_map_table.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_combine{1};
std::atomic<unsigned long long *> g_counters{nullptr};

constexpr int MAX_CAPACITY = 1 << 26;  // slots <= 2^27: a table of 11.8 GB
constexpr int MIN_CAPACITY = 512;      // the table is never smaller than for this capacity: (I)'s rule

int log2_slots(int capacity) {  // of a checked capacity: 10 .. 27
    const int64_t need = 2 * (int64_t)(capacity > MIN_CAPACITY ? capacity : MIN_CAPACITY);
    int l = 10;
    while (((int64_t)1 << l) < need) l++;
    return l;
}

bool capacity_ok(int capacity) { return capacity >= 1 && capacity <= MAX_CAPACITY; }

// The checks of the buffer every device entry makes, and the arguments all kernels share.
const char *check_buffer(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, sv::VoxelMapArgs *a) {
    int nc[3], l;
    if (const char *bad = check_voxel_map("sv_voxel_map", map, map_bytes, spec, nc, &l)) return bad;
    memset(a, 0, sizeof(*a));
    a->map = static_cast<uint8_t *>(map);
    a->log2_slots = l, a->capacity = spec->capacity, a->size = spec->size;
    for (int k = 0; k < 3; k++) a->lo[k] = spec->lo[k], a->hi[k] = spec->hi[k], a->nc[k] = nc[k];
    return nullptr;
}

int launched(hipError_t e) {
    if (e == hipSuccess) return SV_OK;
    sv_internal_set_error("sv_voxel_map: a kernel launch failed");
    return SV_ERR_HIP;
}

}  // namespace

extern "C" {

int64_t sv_voxel_map_slots(int capacity) { return capacity_ok(capacity) ? (int64_t)1 << log2_slots(capacity) : -1; }

size_t sv_voxel_map_bytes(int capacity) { return capacity_ok(capacity) ? sv::vmap_bytes(log2_slots(capacity)) : SIZE_MAX; }

int64_t sv_voxel_map_slot_of(int64_t key, int64_t slots) {
    if (slots < 2 || slots > ((int64_t)1 << 32) || (slots & (slots - 1))) return -1;
    int l = 1;
    while (((int64_t)1 << l) < slots) l++;
    return (int64_t)sv::vmap_slot_of(l, (unsigned long long)key);  // the function the kernels inline
}

int sv_debug_voxel_map(int combine, unsigned long long *counters_device) {
    g_combine.store(combine != 0 ? 1 : 0);
    g_counters.store(counters_device);
    return SV_OK;
}

int sv_voxel_map_clear_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, void *stream) {
    sv::VoxelMapArgs a;
    if (const char *bad = check_buffer(map, map_bytes, spec, &a)) return refuse(bad);
    return launched(sv::launch_voxel_map_clear(a, static_cast<hipStream_t>(stream)));
}

int sv_voxel_map_insert_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const uint8_t *color, const int32_t *n,
                               const int32_t *counts, const double *poses, int batch, int cap, int seq0, void *stream) {
    sv::VoxelMapArgs a;
    if (const char *bad = check_buffer(map, map_bytes, spec, &a)) return refuse(bad);
    if (dtype != SV_CLOUD_F32 && dtype != SV_CLOUD_F64) return refuse("sv_voxel_map: dtype is not SV_CLOUD_F32 / SV_CLOUD_F64");
    if (batch < 0 || batch > 65535) return refuse("sv_voxel_map: batch outside 0..65535");
    if (cap < 0) return refuse("sv_voxel_map: cap < 0");
    if (seq0 < 0 || (int64_t)seq0 + batch > 2147483647ll) return refuse("sv_voxel_map: the sequence numbers must stay in 0 .. 2^31 - 2");
    if (batch > 0 && (!counts || !poses)) return refuse("sv_voxel_map: counts or poses is NULL");
    if (batch > 0 && cap > 0 && !xyz) return refuse("sv_voxel_map: xyz is NULL");
    if (misaligned(xyz, dtype == SV_CLOUD_F32 ? 4 : 8)) return refuse("sv_voxel_map: xyz is not aligned to its element");
    if (misaligned(color, 4) || misaligned(n, 4) || misaligned(counts, 4)) return refuse("sv_voxel_map: color, n or counts is not 4-byte aligned");
    if (misaligned(poses, 8)) return refuse("sv_voxel_map: poses is not 8-byte aligned");
    if (batch == 0 || cap == 0) return SV_OK;
    a.xyz = xyz, a.color = color, a.weight = n, a.counts = counts, a.poses = poses;
    a.cap = cap, a.seq0 = seq0;
    a.counters = g_counters.load();
    return launched(sv::launch_voxel_map_insert(dtype == SV_CLOUD_F32 ? sv::VMAP_F32 : sv::VMAP_F64, g_combine.load() != 0, a, batch, static_cast<hipStream_t>(stream)));
}

int sv_voxel_map_rows_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, int64_t min_n, int64_t min_rows, int since, int dtype, int out_capacity,
                             void *xyz, uint8_t *color, int32_t *cell, int64_t *n, int64_t *m, int32_t *first_seq, int32_t *last_seq, int64_t *key, int32_t *count,
                             void *stream) {
    sv::VoxelMapArgs a;
    if (const char *bad = check_buffer(map, map_bytes, spec, &a)) return refuse(bad);
    if (dtype != SV_CLOUD_F32 && dtype != SV_CLOUD_F64) return refuse("sv_voxel_map: dtype is not SV_CLOUD_F32 / SV_CLOUD_F64");
    if (out_capacity < 0) return refuse("sv_voxel_map: out_capacity < 0");
    if (!count) return refuse("sv_voxel_map: count is NULL");
    if (out_capacity > 0 && (!xyz || !key)) return refuse("sv_voxel_map: xyz or key is NULL");
    if (misaligned(xyz, dtype == SV_CLOUD_F32 ? 4 : 8)) return refuse("sv_voxel_map: xyz is not aligned to its element");
    if (misaligned(color, 4) || misaligned(cell, 4) || misaligned(first_seq, 4) || misaligned(last_seq, 4) || misaligned(count, 4))
        return refuse("sv_voxel_map: color, cell, first_seq, last_seq or count is not 4-byte aligned");
    if (misaligned(n, 8) || misaligned(m, 8) || misaligned(key, 8)) return refuse("sv_voxel_map: n, m or key is not 8-byte aligned");
    a.min_n = min_n, a.min_rows = min_rows, a.since = since, a.out_capacity = out_capacity;
    a.xyz_out = xyz, a.color_out = color, a.cell_out = cell;
    a.n_out = reinterpret_cast<long long *>(n), a.m_out = reinterpret_cast<long long *>(m);
    a.first_out = first_seq, a.last_out = last_seq, a.key_out = reinterpret_cast<long long *>(key), a.count_out = count;
    return launched(sv::launch_voxel_map_rows(dtype == SV_CLOUD_F32 ? sv::VMAP_F32 : sv::VMAP_F64, a, static_cast<hipStream_t>(stream)));
}

} /* extern "C" */
