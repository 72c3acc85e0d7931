// Group (R) of include/stereo_vision_hip.h: a frame's rows matched against the voxel map of (Q) over candidate poses
// (voxel_match_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a
// refused call leaves its text for sv_last_error(NULL).  The check of the map's spec and buffer is stage_glue.h's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_match_kernels.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_group{0};

// NULL for a shape the kernels can index, else what is wrong with it.
const char *check_shape(int cap, int n_poses, int batch) {
    if (cap < 0) return "sv_voxel_match: cap < 0";
    if (batch < 0 || batch > 65535) return "sv_voxel_match: batch outside 0..65535";
    if (n_poses < 1 || n_poses > 65535) return "sv_voxel_match: n_poses outside 1..65535";
    if ((long long)batch * n_poses >= (1ll << 31)) return "sv_voxel_match: batch x n_poses is 2^31 or more";
    return nullptr;
}

int chunks_of(int cap) {
    const long long tiles = ((long long)cap + sv::VMATCH_TILE - 1) / sv::VMATCH_TILE;
    return tiles < 1 ? 1 : tiles > sv::VMATCH_MAX_CHUNKS ? (int)sv::VMATCH_MAX_CHUNKS : (int)tiles;
}

// The two parts of the workspace: the partials, a multiple of 16 bytes, and the group bests.
void layout(int cap, int n_poses, int batch, size_t *partials, size_t *bests) {
    *partials = align16((size_t)batch * chunks_of(cap) * sv::VMATCH_PLANES * (size_t)n_poses * sizeof(unsigned long long));
    *bests = (size_t)batch * sv::VMATCH_GROUPS * sizeof(sv::VoxelMatchBest);
}

}  // namespace

extern "C" {

int sv_voxel_match_workspace(int cap, int n_poses, int batch, size_t *bytes) {
    if (!bytes) return refuse("sv_voxel_match_workspace: bytes is NULL");
    if (const char *bad = check_shape(cap, n_poses, batch)) return refuse(bad);
    size_t p, b;
    layout(cap, n_poses, batch, &p, &b);
    *bytes = p + b;
    return SV_OK;
}

int sv_voxel_match_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const int32_t *n, const int32_t *counts,
                          const double *poses, int batch, int cap, int n_poses, int64_t min_n, int64_t min_rows, int since, int32_t *inside, int32_t *hits,
                          int64_t *weight, int64_t *d2, int32_t *best, int64_t *best_weight, int64_t *best_d2, void *workspace, size_t workspace_bytes, void *stream) {
    int nc[3], l;
    if (const char *bad = check_voxel_map("sv_voxel_match", map, map_bytes, spec, nc, &l)) return refuse(bad);
    if (dtype != SV_CLOUD_F32 && dtype != SV_CLOUD_F64) return refuse("sv_voxel_match: dtype is not SV_CLOUD_F32 / SV_CLOUD_F64");
    if (const char *bad = check_shape(cap, n_poses, batch)) return refuse(bad);
    if (batch > 0 && (!counts || !poses)) return refuse("sv_voxel_match: counts or poses is NULL");
    if (batch > 0 && cap > 0 && !xyz) return refuse("sv_voxel_match: xyz is NULL");
    if (misaligned(xyz, dtype == SV_CLOUD_F32 ? 4 : 8)) return refuse("sv_voxel_match: xyz is not aligned to its element");
    if (misaligned(n, 4) || misaligned(counts, 4)) return refuse("sv_voxel_match: n or counts is not 4-byte aligned");
    if (misaligned(poses, 8)) return refuse("sv_voxel_match: poses is not 8-byte aligned");
    const int given = (inside != nullptr) + (hits != nullptr) + (weight != nullptr) + (d2 != nullptr);
    if (given != 0 && given != 4) return refuse("sv_voxel_match: inside, hits, weight and d2 are given all four or not at all");
    if (batch > 0 && (!best || !best_weight || !best_d2)) return refuse("sv_voxel_match: best, best_weight or best_d2 is NULL");
    if (misaligned(inside, 4) || misaligned(hits, 4) || misaligned(best, 4)) return refuse("sv_voxel_match: inside, hits or best is not 4-byte aligned");
    if (misaligned(weight, 8) || misaligned(d2, 8) || misaligned(best_weight, 8) || misaligned(best_d2, 8))
        return refuse("sv_voxel_match: weight, d2, best_weight or best_d2 is not 8-byte aligned");
    size_t p, b;
    layout(cap, n_poses, batch, &p, &b);
    if (batch > 0 && !workspace) return refuse("sv_voxel_match: the workspace is NULL");
    if (misaligned(workspace, 16)) return refuse("sv_voxel_match: the workspace is not 16-byte aligned");
    if (workspace_bytes < p + b) return refuse("sv_voxel_match: the workspace is smaller than sv_voxel_match_workspace asks for");
    if (batch == 0) return SV_OK;  // nothing to do

    sv::VoxelMatchArgs a;
    memset(&a, 0, sizeof(a));
    a.map = static_cast<const uint8_t *>(map);
    a.log2_slots = l, a.size = spec->size;
    for (int k = 0; k < 3; k++) a.lo[k] = spec->lo[k], a.hi[k] = spec->hi[k], a.nc[k] = nc[k];
    a.xyz = xyz, a.weight = n, a.counts = counts, a.poses = poses;
    a.cap = cap, a.B = batch, a.P = n_poses;
    a.n_chunks = chunks_of(cap);
    a.min_n = min_n, a.min_rows = min_rows, a.since = since;
    char *ws = static_cast<char *>(workspace);
    a.partials = reinterpret_cast<unsigned long long *>(ws);
    a.bests = reinterpret_cast<sv::VoxelMatchBest *>(ws + p);
    a.inside = inside, a.hits = hits, a.weight_out = reinterpret_cast<long long *>(weight), a.d2 = reinterpret_cast<long long *>(d2);
    a.best = best, a.best_weight = reinterpret_cast<long long *>(best_weight), a.best_d2 = reinterpret_cast<long long *>(best_d2);
    // candidates per workgroup: what the test hook asks for, else as many as still leave the chip about 2048 workgroups - the pose words of
    // a candidate are scalar loads, so a small group costs little, and an idle chip costs a lot
    int g = 0;
    if (const int forced = g_group.load()) {
        while ((1 << g) < forced) g++;
    } else {
        for (int k = sv::VMATCH_MAX_LOG_GROUP; k > 0; k--)
            if ((long long)batch * a.n_chunks * ((n_poses + (1 << k) - 1) >> k) >= 2048) {
                g = k;
                break;
            }
    }
    a.log_group = g;
    if (sv::launch_voxel_match(dtype == SV_CLOUD_F32 ? sv::VMAP_F32 : sv::VMAP_F64, a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_match: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_voxel_match(int group) {
    if (group != 0 && (group < 1 || group > (1 << sv::VMATCH_MAX_LOG_GROUP) || (group & (group - 1))))
        return refuse("sv_debug_voxel_match: group must be 0 or a power of two in 1..64");
    g_group.store(group);
    return SV_OK;
}

} /* extern "C" */
