// Group (Y) of include/stereo_vision_hip.h: the surface normals of the voxels of the voxel map of (Q), and a frame's rows paired with the
// nearest voxels and reduced to the sums of one point-to-plane round (voxel_normal_kernels.hip).  Everything here is argument checking and
// launch set-up; every check runs before anything is enqueued, and a refused call leaves its text for sv_last_error(NULL).  The check of
// the map's spec and buffer is stage_glue.h's.
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_normal_kernels.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_max_chunks{0}, g_flags{0};

// NULL for a table of directions and a normal array the kernels can index, else what is wrong with them.
// needed: false for a call that reads neither (an empty batch), which may pass NULL for both.
const char *check_table(const char *prefix, const int8_t *dirs, int n_dirs, const void *normal, int64_t n_normal, int log2_slots, bool needed) {
    if (n_dirs < 1 || n_dirs > sv::VNORMAL_DIRS_MAX) return prefixed(prefix, "n_dirs outside 1..4096");
    if (any_misaligned(4, dirs, normal)) return prefixed(prefix, "dirs or normal is not 4-byte aligned");
    if (needed && (!dirs || !normal)) return prefixed(prefix, "dirs or normal is NULL");
    if ((needed || normal) && n_normal != ((int64_t)1 << log2_slots)) return prefixed(prefix, "normal does not hold one word per slot of the table");
    return nullptr;
}

// NULL for a shape the kernels can index, else what is wrong with it.
const char *check_shape(int cap, int batch) {
    if (cap < 0) return "sv_voxel_plane_align: cap < 0";
    if (batch < 0 || batch > 65535) return "sv_voxel_plane_align: batch outside 0..65535";
    return nullptr;
}

// The row chunks of a frame of `cap` rows, `most` at most.
int chunks_of(int cap, int most) {
    const long long tiles = ((long long)cap + sv::VPLANE_CHUNK - 1) / sv::VPLANE_CHUNK;
    return tiles < 1 ? 1 : tiles > most ? most : (int)tiles;
}

}  // namespace

extern "C" {

int sv_voxel_normals_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const int8_t *dirs, int n_dirs, int min_nb, int flat, int wide, int64_t min_n,
                            int64_t min_rows, int since, int32_t *normal, int64_t n_normal, int64_t *fit, int64_t *counts, void *stream) {
    int nc[3], l;
    if (const char *bad = check_voxel_map("sv_voxel_normals", map, map_bytes, spec, nc, &l)) return refuse(bad);
    if (const char *bad = check_table("sv_voxel_normals", dirs, n_dirs, normal, n_normal, l, true)) return refuse(bad);
    if (min_nb < 3 || min_nb > 27) return refuse("sv_voxel_normals: min_nb outside 3..27");
    if (flat < 0 || flat > 256 || wide < 0 || wide > 256) return refuse("sv_voxel_normals: flat or wide outside 0..256");
    if (!counts) return refuse("sv_voxel_normals: counts is NULL");
    if (misaligned(fit, 8) || misaligned(counts, 8)) return refuse("sv_voxel_normals: fit or counts is not 8-byte aligned");
    const size_t slots = (size_t)1 << l;
    const Span spans[] = {{map, map_bytes}, {dirs, (size_t)n_dirs * 4}, {normal, slots * 4}, {fit, fit ? slots * 32 : 0}, {counts, 32}};
    if (outputs_overlap(spans, 5, 2)) return refuse("sv_voxel_normals: an output shares a byte with the map, the table or another output");

    sv::VoxelNormalArgs a;
    memset(&a, 0, sizeof(a));
    a.map = static_cast<const uint8_t *>(map);
    a.log2_slots = l;
    for (int k = 0; k < 3; k++) a.nc[k] = nc[k];
    a.dirs = dirs, a.K = n_dirs;
    a.min_nb = min_nb, a.flat = flat, a.wide = wide, a.flags = g_flags.load();
    a.min_n = min_n < 1 ? 1 : min_n, a.min_rows = min_rows, a.since = since;  // a tombstone (n = 0) is never a member
    a.normal = normal, a.fit = reinterpret_cast<long long *>(fit), a.counts = reinterpret_cast<unsigned long long *>(counts);
    if (sv::launch_voxel_normals(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_normals: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_voxel_plane_align_workspace(int cap, int batch, size_t *bytes) {
    if (!bytes) return refuse("sv_voxel_plane_align_workspace: bytes is NULL");
    if (const char *bad = check_shape(cap, batch)) return refuse(bad);
    *bytes = (size_t)batch * chunks_of(cap, sv::VPLANE_MAX_CHUNKS) * sv::VPLANE_WORDS * sizeof(unsigned long long);
    return SV_OK;
}

int sv_voxel_plane_align_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const int32_t *n, const int32_t *counts,
                                const double *poses, const int32_t *origin, int batch, int cap, int max_d2, int64_t min_n, int64_t min_rows, int since, const int32_t *normal,
                                int64_t n_normal, const int8_t *dirs, int n_dirs, int64_t *sums, int64_t *pair_key, int32_t *pair_d2, int32_t *pair_normal, void *workspace,
                                size_t workspace_bytes, void *stream) {
    int nc[3], l;
    if (const char *bad = check_voxel_map("sv_voxel_plane_align", map, map_bytes, spec, nc, &l)) return refuse(bad);
    if (dtype != SV_CLOUD_F32 && dtype != SV_CLOUD_F64) return refuse("sv_voxel_plane_align: dtype is not SV_CLOUD_F32 / SV_CLOUD_F64");
    if (const char *bad = check_shape(cap, batch)) return refuse(bad);
    if (max_d2 < 0 || max_d2 > sv::VPLANE_D2_MAX) return refuse("sv_voxel_plane_align: max_d2 outside 0..783363");
    if (const char *bad = check_table("sv_voxel_plane_align", dirs, n_dirs, normal, n_normal, l, batch > 0)) return refuse(bad);
    if (batch > 0 && (!counts || !poses || !origin)) return refuse("sv_voxel_plane_align: counts, poses or origin is NULL");
    if (batch > 0 && cap > 0 && !xyz) return refuse("sv_voxel_plane_align: xyz is NULL");
    if (misaligned(xyz, dtype == SV_CLOUD_F32 ? 4 : 8)) return refuse("sv_voxel_plane_align: xyz is not aligned to its element");
    if (any_misaligned(4, n, counts, origin)) return refuse("sv_voxel_plane_align: n, counts or origin is not 4-byte aligned");
    if (misaligned(poses, 8)) return refuse("sv_voxel_plane_align: poses is not 8-byte aligned");
    if (batch > 0 && !sums) return refuse("sv_voxel_plane_align: sums is NULL");
    if ((pair_key != nullptr) != (pair_d2 != nullptr) || (pair_key != nullptr) != (pair_normal != nullptr))
        return refuse("sv_voxel_plane_align: pair_key, pair_d2 and pair_normal are given all or not at all");
    if (misaligned(sums, 8) || misaligned(pair_key, 8)) return refuse("sv_voxel_plane_align: sums or pair_key is not 8-byte aligned");
    if (any_misaligned(4, pair_d2, pair_normal)) return refuse("sv_voxel_plane_align: pair_d2 or pair_normal is not 4-byte aligned");
    size_t need;
    sv_voxel_plane_align_workspace(cap, batch, &need);
    if (batch > 0 && !workspace) return refuse("sv_voxel_plane_align: the workspace is NULL");
    if (misaligned(workspace, 8)) return refuse("sv_voxel_plane_align: the workspace is not 8-byte aligned");
    if (workspace_bytes < need) return refuse("sv_voxel_plane_align: the workspace is smaller than sv_voxel_plane_align_workspace asks for");
    if (batch == 0) return SV_OK;  // nothing to do

    sv::VoxelPlaneArgs a;
    memset(&a, 0, sizeof(a));
    a.map = static_cast<const uint8_t *>(map);
    a.log2_slots = l, a.size = spec->size;
    for (int k = 0; k < 3; k++) a.lo[k] = spec->lo[k], a.hi[k] = spec->hi[k], a.nc[k] = nc[k];
    a.xyz = xyz, a.weight = n, a.counts = counts, a.poses = poses, a.origin = origin;
    a.normal = normal, a.dirs = dirs, a.K = n_dirs;
    a.cap = cap, a.B = batch;
    const int most = g_max_chunks.load();
    a.n_chunks = chunks_of(cap, most ? most : (int)sv::VPLANE_MAX_CHUNKS);
    a.max_d2 = max_d2, a.flags = g_flags.load();
    a.min_n = min_n < 1 ? 1 : min_n, a.min_rows = min_rows, a.since = since;  // a tombstone (n = 0) is never a partner
    a.partials = static_cast<unsigned long long *>(workspace);
    a.sums = reinterpret_cast<long long *>(sums);
    a.pair_key = reinterpret_cast<long long *>(pair_key), a.pair_d2 = pair_d2, a.pair_normal = pair_normal;
    if (sv::launch_voxel_plane_align(dtype == SV_CLOUD_F32 ? sv::VMAP_F32 : sv::VMAP_F64, a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_plane_align: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_voxel_normals(int max_chunks, int flags) {
    if (max_chunks < 0 || max_chunks > sv::VPLANE_MAX_CHUNKS) return refuse("sv_debug_voxel_normals: max_chunks must be 0 or in 1..512");
    if (flags & ~(int)(sv::VPLANE_NO_SKIP | sv::VNORMAL_NO_PRUNE)) return refuse("sv_debug_voxel_normals: flags has an unknown bit");
    g_max_chunks.store(max_chunks);
    g_flags.store(flags);
    return SV_OK;
}

} /* extern "C" */
