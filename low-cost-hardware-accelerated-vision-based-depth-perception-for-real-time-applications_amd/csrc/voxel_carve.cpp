// Group (T) of include/stereo_vision_hip.h: a voxel map of (Q) carved by the sight lines of frames (voxel_carve_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).  The check of a map's spec and buffer is stage_glue.h's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_carve_kernels.h"

namespace {

using namespace sv::glue;

}  // namespace

extern "C" {

int sv_voxel_carve_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const int32_t *n, const int32_t *counts,
                          const double *poses, const double *origin, int batch, int cap, int seq0, int reach, int margin, int64_t min_miss, int ratio, int apply,
                          uint64_t *miss, int64_t *stats, void *stream) {
    int nc[3], l;
    if (const char *bad = check_voxel_map("sv_voxel_carve", map, map_bytes, spec, nc, &l)) return refuse(bad);
    if (dtype != SV_CLOUD_F32 && dtype != SV_CLOUD_F64) return refuse("sv_voxel_carve: dtype is not SV_CLOUD_F32 / SV_CLOUD_F64");
    if (batch < 0 || batch > 65535) return refuse("sv_voxel_carve: batch outside 0..65535");
    if (cap < 0) return refuse("sv_voxel_carve: cap < 0");
    if (seq0 < 0 || (int64_t)seq0 + batch > 2147483647ll) return refuse("sv_voxel_carve: the sequence numbers must stay in 0 .. 2^31 - 2");
    if (reach < 1 || reach > sv::VCARVE_REACH_MAX) return refuse("sv_voxel_carve: reach outside 1..1023");
    if (margin < 0 || margin > sv::VCARVE_MARGIN_MAX) return refuse("sv_voxel_carve: margin outside 0..255");
    if (min_miss < 1) return refuse("sv_voxel_carve: min_miss < 1");
    if (ratio < 0 || ratio > 65535) return refuse("sv_voxel_carve: ratio outside 0..65535");
    if (apply != 0 && apply != 1) return refuse("sv_voxel_carve: apply is not 0 or 1");
    if (batch > 0 && (!counts || !poses)) return refuse("sv_voxel_carve: counts or poses is NULL");
    if (batch > 0 && cap > 0 && !xyz) return refuse("sv_voxel_carve: xyz is NULL");
    if (misaligned(xyz, dtype == SV_CLOUD_F32 ? 4 : 8)) return refuse("sv_voxel_carve: xyz is not aligned to its element");
    if (misaligned(n, 4) || misaligned(counts, 4)) return refuse("sv_voxel_carve: n or counts is not 4-byte aligned");
    if (misaligned(poses, 8)) return refuse("sv_voxel_carve: poses is not 8-byte aligned");
    if (!origin) return refuse("sv_voxel_carve: origin is NULL");
    for (int k = 0; k < 3; k++)
        if (!isfinite(origin[k])) return refuse("sv_voxel_carve: origin is not finite");
    if (!miss || misaligned(miss, 8)) return refuse("sv_voxel_carve: miss is NULL or not 8-byte aligned");
    if (misaligned(stats, 8)) return refuse("sv_voxel_carve: stats is not 8-byte aligned");
    const size_t miss_bytes = ((size_t)1 << l) * sizeof(uint64_t), stats_bytes = sv::VCARVE_STATS * sizeof(int64_t);
    if (overlap(miss, miss_bytes, map, map_bytes) || overlap(stats, stats_bytes, map, map_bytes)) return refuse("sv_voxel_carve: miss or stats lies inside the map");
    if (overlap(miss, miss_bytes, stats, stats_bytes)) return refuse("sv_voxel_carve: miss and stats overlap");

    sv::VoxelCarveArgs a;
    memset(&a, 0, sizeof(a));
    a.map = static_cast<uint8_t *>(map);
    a.log2_slots = l, a.size = spec->size;
    for (int k = 0; k < 3; k++) a.lo[k] = spec->lo[k], a.hi[k] = spec->hi[k], a.nc[k] = nc[k], a.origin[k] = origin[k];
    a.xyz = xyz, a.weight = n, a.counts = counts, a.poses = poses;
    a.cap = cap, a.seq0 = seq0, a.reach = reach, a.margin = margin, a.min_miss = min_miss, a.ratio = ratio, a.apply = apply;
    a.miss = reinterpret_cast<unsigned long long *>(miss), a.stats = reinterpret_cast<long long *>(stats);
    if (sv::launch_voxel_carve(dtype == SV_CLOUD_F32 ? sv::VMAP_F32 : sv::VMAP_F64, a, batch, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_carve: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
