// Group (W) of include/stereo_vision_hip.h: the connected components of a voxel map of (Q) (voxel_cluster_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).  The checks of the voxel map's spec and buffer and of the flat map's spec are stage_glue.h's.
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_cluster_kernels.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_groups{0};  // sv_debug_voxel_clusters: the workgroups of a table walk at most, 0 = VCLUSTER_MAX_GROUPS
std::atomic<int> g_stages{0};  // and the kernels a call enqueues (the low four bits, 0 = all) with the two choices above them

}  // namespace

extern "C" {

size_t sv_voxel_clusters_workspace_bytes(int64_t capacity_of_map, int capacity) {
    if (capacity < 1 || capacity > sv::VCLUSTER_CAPACITY_MAX || capacity_of_map < 1 || capacity_of_map > (1 << 26)) return 0;
    const int64_t slots = sv_voxel_map_slots((int)capacity_of_map);
    return slots > 0 ? sv::voxel_cluster_workspace_words((size_t)slots) * sizeof(int32_t) : 0;
}

int sv_voxel_clusters_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const sv_voxel_cluster_spec *cluster, const sv_occupancy_map_spec *flat,
                             const int32_t *floor, int64_t min_n, int64_t min_rows, int since, int32_t *label, int64_t *clusters, int64_t *info, void *workspace,
                             size_t workspace_bytes, void *stream) {
    int nc[3], l;
    if (const char *bad = check_voxel_map("sv_voxel_clusters", map, map_bytes, spec, nc, &l)) return refuse(bad);
    if (!cluster) return refuse("sv_voxel_clusters: cluster is NULL");
    for (int k = 0; k < 8; k++)
        if (cluster->reserved[k] != 0) return refuse("sv_voxel_clusters: a reserved word of cluster is not 0");
    if (cluster->connectivity != 6 && cluster->connectivity != 18 && cluster->connectivity != 26) return refuse("sv_voxel_clusters: connectivity is none of 6, 18, 26");
    if (cluster->mode != 0 && cluster->mode != 1) return refuse("sv_voxel_clusters: mode is neither 0 nor 1");
    if (cluster->mode == 0 && (cluster->z_ref_q < -sv::VCLUSTER_BAND_MAX || cluster->z_ref_q > sv::VCLUSTER_BAND_MAX)) return refuse("sv_voxel_clusters: |z_ref_q| above 2^30");
    if (!(-sv::VCLUSTER_BAND_MAX <= cluster->h_lo_q && cluster->h_lo_q < cluster->h_hi_q && cluster->h_hi_q <= sv::VCLUSTER_BAND_MAX))
        return refuse("sv_voxel_clusters: the band needs -2^30 <= h_lo_q < h_hi_q <= 2^30");
    if (cluster->min_voxels < 1) return refuse("sv_voxel_clusters: min_voxels < 1");
    if (cluster->capacity < 1 || cluster->capacity > sv::VCLUSTER_CAPACITY_MAX) return refuse("sv_voxel_clusters: capacity outside 1..65535");
    if (cluster->drop != 0 && cluster->drop != 1) return refuse("sv_voxel_clusters: drop is neither 0 nor 1");
    if (cluster->mode == 1) {
        if (const char *bad = check_map("sv_voxel_clusters", flat)) return refuse(bad);
        if (!floor) return refuse("sv_voxel_clusters: floor is NULL in mode 1");
        if (misaligned(floor, 4)) return refuse("sv_voxel_clusters: floor is not 4-byte aligned");
    }
    if (min_n < 1) return refuse("sv_voxel_clusters: min_n < 1");
    if (!label || !clusters || !info || !workspace) return refuse("sv_voxel_clusters: label, clusters, info or workspace is NULL");
    if (any_misaligned(8, clusters, info)) return refuse("sv_voxel_clusters: clusters or info is not 8-byte aligned");
    if (misaligned(label, 4) || misaligned(workspace, 4)) return refuse("sv_voxel_clusters: label or workspace is not 4-byte aligned");
    const size_t slots = (size_t)1 << l, ws_words = sv::voxel_cluster_workspace_words(slots);
    if (workspace_bytes < ws_words * sizeof(int32_t)) return refuse("sv_voxel_clusters: workspace_bytes below sv_voxel_clusters_workspace_bytes");
    const size_t n_floor = cluster->mode == 1 ? (size_t)flat->rows * flat->cols * 4 : 0;
    const Span spans[] = {{map, map_bytes}, {floor, n_floor}, {label, slots * 4}, {clusters, (size_t)cluster->capacity * sv::VCLUSTER_ROW_WORDS * 8},
                          {info, sv::VCLUSTER_INFO * sizeof(int64_t)}, {workspace, ws_words * sizeof(int32_t)}};
    if (outputs_overlap(spans, 6, 2)) return refuse("sv_voxel_clusters: an output or the workspace shares a byte with the map, the floor or another output");

    sv::VoxelClusterArgs a;
    memset(&a, 0, sizeof(a));
    a.map = static_cast<uint8_t *>(map);
    a.log2_slots = l, a.size = spec->size;
    for (int k = 0; k < 3; k++) a.lo[k] = spec->lo[k], a.nc[k] = nc[k];
    a.min_n = min_n, a.min_rows = min_rows, a.since = since;
    a.connectivity = cluster->connectivity, a.mode = cluster->mode, a.z_ref_q = cluster->mode == 0 ? cluster->z_ref_q : 0;
    a.h_lo_q = cluster->h_lo_q, a.h_hi_q = cluster->h_hi_q, a.min_voxels = cluster->min_voxels, a.capacity = cluster->capacity, a.drop = cluster->drop;
    if (cluster->mode == 1) a.m = sv::map_cells_of(*flat), a.floor = floor;
    a.label = label, a.clusters = reinterpret_cast<long long *>(clusters), a.info = reinterpret_cast<long long *>(info);
    a.parent = static_cast<int32_t *>(workspace), a.count = a.parent + slots, a.blocks = a.count + slots;
    const int groups = g_groups.load(), stages = g_stages.load();
    a.flags = stages & (sv::VCLUSTER_NO_COMBINE | sv::VCLUSTER_NO_COMPRESS);
    if (sv::launch_voxel_clusters(a, groups ? groups : sv::VCLUSTER_MAX_GROUPS, stages & 15, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_clusters: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_voxel_clusters(int groups, int stages) {
    if (stages >= 0 && stages < 64 && (stages & 15) < sv::VCLUSTER_STAGES) g_stages.store(stages);
    if (groups < 0 || groups > sv::VCLUSTER_MAX_GROUPS) return g_groups.load();
    return g_groups.exchange(groups);
}

} /* extern "C" */
