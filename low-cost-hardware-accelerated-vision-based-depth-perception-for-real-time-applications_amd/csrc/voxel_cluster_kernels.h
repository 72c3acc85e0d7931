// Launch interface of voxel_cluster_kernels.hip (the connected components of a voxel map: voxel_cluster.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_map_cells.h"  // the flat map's geometry: MapCells
#include "voxel_map_kernels.h"    // the voxel map's buffer: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES

namespace sv {

enum {
    VCLUSTER_THREADS = 256,       // a workgroup of every kernel here: four wavefronts
    VCLUSTER_MAX_GROUPS = 2048,   // workgroups of a table walk at most: a larger table is walked in strides
    VCLUSTER_WAVE_SLOTS = 1024,   // the slots a wavefront owns in count and rank: a table has a multiple of them
    VCLUSTER_CAPACITY_MAX = 65535,
    VCLUSTER_ROW_WORDS = 16,      // int64 words of a cluster row
    VCLUSTER_INFO = 8,            // members, components, kept, small voxels, emptied, largest, 0, 0
    VCLUSTER_BAND_MAX = 1 << 30,  // |z_ref_q|, |h_lo_q| and |h_hi_q| at most
    VCLUSTER_STAGES = 8,          // init, link, roots, count, scan, rank, stats, resolve
    VCLUSTER_NO_COMBINE = 16,     // flags of launch_voxel_clusters: roots and stats issue one atomic per member
    VCLUSTER_NO_COMPRESS = 32     // the link kernel leaves a member's own word where the unions put it: no path compression
};

struct VoxelClusterArgs {
    uint8_t *map;    // only read unless drop
    int log2_slots;  // 10 .. 27
    double lo[3], size;
    int nc[3];                  // the cells per axis: 1 .. 2^20
    long long min_n, min_rows;  // min_n >= 1
    int since;
    int connectivity;            // 6, 18 or 26
    int mode, z_ref_q;           // 0: base = z_ref_q; 1: base = floor[cell]
    int h_lo_q, h_hi_q;          // the band, h_lo_q <= zq - base < h_hi_q
    int min_voxels, capacity;    // >= 1; 1 .. VCLUSTER_CAPACITY_MAX
    int drop, flags;
    MapCells m;                  // mode 1: the flat map's
    const int32_t *floor;        // mode 1: [rows][cols], only read
    int32_t *label;              // [slots]: the root's slot between roots and resolve
    long long *clusters;         // [capacity][VCLUSTER_ROW_WORDS]
    long long *info;             // [VCLUSTER_INFO]
    int32_t *parent, *count;     // workspace, [slots] each; count holds a root's count, then its row, -2 or -3
    int32_t *blocks;             // workspace, [2 * slots / VCLUSTER_WAVE_SLOTS]: kept roots per wavefront, their prefix
};

// int32 words of the workspace of a table of `slots` entries.
inline size_t voxel_cluster_workspace_words(size_t slots) { return 2 * slots + 2 * (slots / VCLUSTER_WAVE_SLOTS); }

// Eight kernels in stream order.  max_groups in 1 .. VCLUSTER_MAX_GROUPS: the workgroups of a walk (init, link, roots, stats, resolve).
// stages: 0 = all, 1 .. 7 = the first that many only (a measurement hook).  a.flags: VCLUSTER_NO_COMBINE | VCLUSTER_NO_COMPRESS.
hipError_t launch_voxel_clusters(const VoxelClusterArgs &a, int max_groups, int stages, hipStream_t st);

}  // namespace sv
