// Group (N) of include/stereo_vision_hip.h: the penalties made from the clearance field, the cost-to-goal field of the world map and the
// routes traced through it (cost_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything
// is enqueued, a refused call leaves its text for sv_last_error(NULL), and no entry waits for the GPU.
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "cost_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_variant{sv::COST_DIRTY_TILES};
std::atomic<unsigned long long *> g_counters{nullptr};

// NULL for a map the field's int32 costs can hold, else what is wrong with it.
const char *check_cells(const char *prefix, int rows, int cols) {
    if (const char *bad = check_map_shape(prefix, rows, cols)) return bad;
    if ((int64_t)rows * cols > sv::COST_CELLS_MAX) return prefixed(prefix, "rows * cols above 8 000 000, where a cost could reach 2^31 - 1");
    return nullptr;
}

// The workspace of the field: the sweeps' words first - the block the call's memset clears - then the twin buffer and the dirty bytes.
struct Layout {
    size_t words, twin, dirty, total;
    int tiles_x, tiles_y;
};

Layout layout_of(int rows, int cols) {
    Layout l;
    l.tiles_x = (cols + sv::COST_TILE - 1) / sv::COST_TILE, l.tiles_y = (rows + sv::COST_TILE - 1) / sv::COST_TILE;
    l.words = align16(sv::COST_SWEEPS_MAX * sizeof(int32_t));
    l.twin = align16((size_t)rows * cols * sizeof(int32_t));
    l.dirty = align16((size_t)l.tiles_x * l.tiles_y);
    l.total = l.words + l.twin + 2 * l.dirty;
    return l;
}

}  // namespace

extern "C" {

int sv_cost_cells_device(const uint16_t *d2, int rows, int cols, int radius, int r2_block, int soft, int weight, uint8_t *pen, void *stream) {
    if (!d2 || !pen) return refuse("sv_cost_cells: d2 or pen is NULL");
    if (const char *bad = check_map_shape("sv_cost_cells", rows, cols)) return refuse(bad);
    if (radius < 1 || radius > 254) return refuse("sv_cost_cells: radius outside 1..254");
    if (r2_block < 0 || r2_block > radius * radius) return refuse("sv_cost_cells: r2_block is negative or above radius^2, where a saturated cell would hide an obstacle");
    if (soft < 0 || soft > sv::COST_PEN_MAX || weight < 0 || weight > sv::COST_PEN_MAX) return refuse("sv_cost_cells: soft or weight outside 0..254");
    if (misaligned(d2, 2)) return refuse("sv_cost_cells: d2 is not 2-byte aligned");
    const size_t cells = (size_t)rows * cols;
    if (overlap(pen, cells, d2, cells * 2)) return refuse("sv_cost_cells: pen overlaps d2");

    sv::CostCellsArgs a;
    memset(&a, 0, sizeof(a));
    a.d2 = d2, a.pen = pen, a.cells = (int64_t)cells, a.r2_block = r2_block, a.soft = soft, a.weight = weight;
    if (sv::launch_cost_cells(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_cost_cells: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_cost_to_goal_workspace(int rows, int cols, size_t *bytes) {
    if (!bytes) return refuse("sv_cost_to_goal_workspace: bytes is NULL");
    if (const char *bad = check_cells("sv_cost_to_goal_workspace", rows, cols)) return refuse(bad);
    *bytes = layout_of(rows, cols).total;
    return SV_OK;
}

int sv_cost_to_goal_device(const uint8_t *pen, int rows, int cols, const int32_t *goals, int n_goals, int init, int sweeps, int32_t *cost, void *workspace,
                           size_t workspace_bytes, int32_t *info, void *stream) {
    if (!pen || !goals || !cost || !workspace || !info) return refuse("sv_cost_to_goal: pen, goals, cost, the workspace or info is NULL");
    if (const char *bad = check_cells("sv_cost_to_goal", rows, cols)) return refuse(bad);
    if (n_goals < 1 || n_goals > sv::COST_GOALS_MAX) return refuse("sv_cost_to_goal: n_goals outside 1..1024");
    if (init != 0 && init != 1) return refuse("sv_cost_to_goal: init is neither 0 nor 1");
    if (sweeps < 2 || sweeps > sv::COST_SWEEPS_MAX || (sweeps & 1)) return refuse("sv_cost_to_goal: sweeps is odd or outside 2..1024");
    if (any_misaligned(4, goals, cost, info))
        return refuse("sv_cost_to_goal: goals, cost or info is not 4-byte aligned");
    if (misaligned(workspace, 16)) return refuse("sv_cost_to_goal: the workspace is not 16-byte aligned");
    const Layout l = layout_of(rows, cols);
    if (workspace_bytes < l.total) return refuse("sv_cost_to_goal: the workspace is smaller than sv_cost_to_goal_workspace asks for");
    const size_t cells = (size_t)rows * cols, goal_bytes = (size_t)n_goals * 8;
    const Span spans[5] = {{pen, cells}, {goals, goal_bytes}, {cost, cells * 4}, {info, 16}, {workspace, l.total}};
    if (outputs_overlap(spans, 5, 2))  // cost is the first output
        return refuse("sv_cost_to_goal: cost, info and the workspace overlap one another, pen or goals");

    sv::CostFieldArgs a;
    memset(&a, 0, sizeof(a));
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    a.pen = pen, a.goals = goals, a.cost = cost, a.info = info;
    a.changed = reinterpret_cast<int32_t *>(ws);
    a.twin = reinterpret_cast<int32_t *>(ws + l.words);
    a.dirty[0] = ws + l.words + l.twin, a.dirty[1] = a.dirty[0] + l.dirty;
    a.counters = g_counters.load();
    a.rows = rows, a.cols = cols, a.tiles_x = l.tiles_x, a.tiles_y = l.tiles_y, a.n_goals = n_goals;
    a.all_tiles = g_variant.load() == sv::COST_ALL_TILES;
    if (sv::launch_cost_to_goal(a, init, sweeps, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_cost_to_goal: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_cost_routes_device(const int32_t *cost, const uint8_t *pen, int rows, int cols, const int32_t *starts, int n_routes, int capacity, int16_t *cells,
                          int32_t *length, int32_t *status, void *stream) {
    if (const char *bad = check_cells("sv_cost_routes", rows, cols)) return refuse(bad);
    if (n_routes < 0 || n_routes > 65535) return refuse("sv_cost_routes: n_routes outside 0..65535");
    if (capacity < 1 || capacity > 65535) return refuse("sv_cost_routes: capacity outside 1..65535");
    if (!cost || !pen) return refuse("sv_cost_routes: cost or pen is NULL");
    if (n_routes > 0 && (!starts || !cells || !length || !status)) return refuse("sv_cost_routes: starts, cells, length or status is NULL");
    if (any_misaligned(4, cost, starts, cells, length, status))
        return refuse("sv_cost_routes: cost, starts, cells, length or status is not 4-byte aligned");
    if (n_routes == 0) return SV_OK;  // nothing to do
    const size_t map_cells = (size_t)rows * cols, k = (size_t)n_routes, cell_bytes = k * capacity * 4;
    const Span spans[6] = {{cost, map_cells * 4}, {pen, map_cells}, {starts, k * 8}, {cells, cell_bytes}, {length, k * 4}, {status, k * 4}};
    if (outputs_overlap(spans, 6, 3))  // cells is the first output
        return refuse("sv_cost_routes: an output overlaps an input or another output");

    sv::CostRoutesArgs a;
    memset(&a, 0, sizeof(a));
    a.cost = cost, a.pen = pen, a.starts = starts, a.cells = cells, a.length = length, a.status = status;
    a.rows = rows, a.cols = cols, a.n_routes = n_routes, a.capacity = capacity;
    if (sv::launch_cost_routes(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_cost_routes: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_cost_to_goal(int variant, unsigned long long *counters_device) {
    if (variant != sv::COST_DIRTY_TILES && variant != sv::COST_ALL_TILES) return refuse("sv_debug_cost_to_goal: variant must be 0 (the dirty tiles) or 1 (every tile)");
    g_variant.store(variant);
    g_counters.store(counters_device);
    return SV_OK;
}

} /* extern "C" */
