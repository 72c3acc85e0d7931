// Group (O) of include/stereo_vision_hip.h: the frontier cells of the world map and their connected clusters (frontier_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, a refused call leaves its text
// for sv_last_error(NULL), and no entry waits for the GPU.
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "frontier_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_variant{sv::FRONTIER_TILES};
std::atomic<unsigned long long *> g_counters{nullptr};

// NULL for a map whose linear indices fit 23 bits and a table of rows the kernels can index, else what is wrong with them.
const char *check_shape(const char *prefix, int rows, int cols, int capacity) {
    if (const char *bad = check_map_shape(prefix, rows, cols)) return bad;
    if ((int64_t)rows * cols > sv::FRONTIER_CELLS_MAX) return prefixed(prefix, "rows * cols above 8 000 000, where a linear index could reach 2^23");
    if (capacity < 1 || capacity > sv::FRONTIER_CAPACITY_MAX) return prefixed(prefix, "capacity outside 1..65535");
    return nullptr;
}

// The workspace of the clusters: the roots' counts first - the block the first memset clears -, the keys of the representatives - the
// block the second one fills -, then the parents and the words of the compaction.
struct Layout {
    size_t size, key, parent, blocks, total;
    int tiles_x, tiles_y, n_blocks;
};

Layout layout_of(int rows, int cols, int capacity) {
    Layout l;
    const size_t cells = (size_t)rows * cols;
    l.tiles_x = (cols + sv::FRONTIER_TILE - 1) / sv::FRONTIER_TILE, l.tiles_y = (rows + sv::FRONTIER_TILE - 1) / sv::FRONTIER_TILE;
    l.n_blocks = (int)((cells + 1023) / 1024);
    l.size = align16(cells * sizeof(int32_t));
    l.key = align16((size_t)capacity * sizeof(unsigned long long));
    l.parent = align16(cells * sizeof(int32_t));
    l.blocks = align16((size_t)l.n_blocks * 4 * sizeof(int32_t));
    l.total = l.size + l.key + l.parent + l.blocks;
    return l;
}

}  // namespace

extern "C" {

int sv_frontier_cells_device(const int16_t *logodds, const int32_t *last_seen, const uint8_t *pen, int rows, int cols, int occupied, int free_, uint8_t *mask,
                             void *stream) {
    if (!logodds || !last_seen || !mask) return refuse("sv_frontier_cells: logodds, last_seen or mask is NULL");
    if (const char *bad = check_map_shape("sv_frontier_cells", rows, cols)) return refuse(bad);
    if (misaligned(logodds, 2)) return refuse("sv_frontier_cells: logodds is not 2-byte aligned");
    if (misaligned(last_seen, 4)) return refuse("sv_frontier_cells: last_seen is not 4-byte aligned");
    const size_t cells = (size_t)rows * cols;
    if (overlap(mask, cells, logodds, cells * 2) || overlap(mask, cells, last_seen, cells * 4) || overlap(mask, cells, pen, cells))
        return refuse("sv_frontier_cells: mask overlaps logodds, last_seen or pen");

    sv::FrontierCellsArgs a;
    memset(&a, 0, sizeof(a));
    a.logodds = logodds, a.last_seen = last_seen, a.pen = pen, a.mask = mask, a.rows = rows, a.cols = cols, a.occupied = occupied, a.free_ = free_;
    if (sv::launch_frontier_cells(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_frontier_cells: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_frontier_clusters_workspace(int rows, int cols, int capacity, size_t *bytes) {
    if (!bytes) return refuse("sv_frontier_clusters_workspace: bytes is NULL");
    if (const char *bad = check_shape("sv_frontier_clusters_workspace", rows, cols, capacity)) return refuse(bad);
    *bytes = layout_of(rows, cols, capacity).total;
    return SV_OK;
}

int sv_frontier_clusters_device(const uint8_t *mask, int rows, int cols, int min_cells, int capacity, int32_t *label, int32_t *clusters, int64_t *sums, int32_t *info,
                                void *workspace, size_t workspace_bytes, void *stream) {
    if (!mask || !label || !clusters || !sums || !info || !workspace) return refuse("sv_frontier_clusters: mask, label, clusters, sums, info or the workspace is NULL");
    if (const char *bad = check_shape("sv_frontier_clusters", rows, cols, capacity)) return refuse(bad);
    if (min_cells < 1 || min_cells > sv::FRONTIER_CELLS_MAX) return refuse("sv_frontier_clusters: min_cells outside 1..8 000 000");
    if (any_misaligned(4, label, clusters, info))
        return refuse("sv_frontier_clusters: label, clusters or info is not 4-byte aligned");
    if (misaligned(sums, 8)) return refuse("sv_frontier_clusters: sums is not 8-byte aligned");
    if (misaligned(workspace, 16)) return refuse("sv_frontier_clusters: the workspace is not 16-byte aligned");
    const Layout l = layout_of(rows, cols, capacity);
    if (workspace_bytes < l.total) return refuse("sv_frontier_clusters: the workspace is smaller than sv_frontier_clusters_workspace asks for");
    const size_t cells = (size_t)rows * cols;
    const Span spans[6] = {{mask, cells}, {label, cells * 4}, {clusters, (size_t)capacity * 32}, {sums, (size_t)capacity * 16}, {info, 16}, {workspace, l.total}};
    if (outputs_overlap(spans, 6, 1))  // mask is the only input
        return refuse("sv_frontier_clusters: label, clusters, sums, info and the workspace overlap one another or mask");

    sv::FrontierArgs a;
    memset(&a, 0, sizeof(a));
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    a.mask = mask, a.label = label, a.clusters = clusters, a.sums = reinterpret_cast<long long *>(sums), a.info = info;
    a.size = reinterpret_cast<int32_t *>(ws);
    a.key = reinterpret_cast<unsigned long long *>(ws + l.size);
    a.parent = reinterpret_cast<int32_t *>(ws + l.size + l.key);
    a.blocks = reinterpret_cast<int32_t *>(ws + l.size + l.key + l.parent);
    a.counters = g_counters.load();
    a.rows = rows, a.cols = cols, a.tiles_x = l.tiles_x, a.tiles_y = l.tiles_y, a.n_blocks = l.n_blocks, a.min_cells = min_cells, a.capacity = capacity;
    a.no_tiles = g_variant.load() == sv::FRONTIER_NO_TILES;
    if (sv::launch_frontier_clusters(a, l.size, l.key, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_frontier_clusters: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_frontier(int variant, unsigned long long *counters_device) {
    if (variant != sv::FRONTIER_TILES && variant != sv::FRONTIER_NO_TILES)
        return refuse("sv_debug_frontier: variant must be 0 (tiles, then their seams) or 1 (no tile phase)");
    g_variant.store(variant);
    g_counters.store(counters_device);
    return SV_OK;
}

} /* extern "C" */
