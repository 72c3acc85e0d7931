// Group (I) of include/stereo_vision_hip.h: voxel-grid downsampled clouds from disparity maps (voxel_kernels.hip).  Everything here is
// argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its text for
// sv_last_error(NULL).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_kernels.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_combine{1};
std::atomic<unsigned long long *> g_counters{nullptr};

constexpr int MAX_CAPACITY = 1 << 26;  // slots <= 2^27: a table of 9.7 GB per pair, and every launch below 2^32 threads per row

// NULL for a good spec and good sizes, else what is wrong with them; nc = the cells per axis of a good spec.
const char *check_shape(const sv_voxel_spec *s, int batch, int width, int height, int *nc) {
    if (!s) return "sv_voxel: spec is NULL";
    for (int k = 0; k < 5; k++)
        if (s->reserved[k] != 0) return "sv_voxel: a reserved word of the spec is not 0";
    if (s->disparity != SV_CLOUD_DMAP && s->disparity != SV_CLOUD_D1) return "sv_voxel: disparity is not SV_CLOUD_DMAP / SV_CLOUD_D1";
    if (s->dtype != SV_CLOUD_F32 && s->dtype != SV_CLOUD_F64) return "sv_voxel: dtype is not SV_CLOUD_F32 / SV_CLOUD_F64";
    if (s->step < 1) return "sv_voxel: step < 1";
    if (!(s->size > 0.0) || !isfinite(s->size)) return "sv_voxel: size is not a finite number > 0";
    for (int k = 0; k < 3; k++) {
        if (!isfinite(s->lo[k]) || !isfinite(s->hi[k])) return "sv_voxel: the crop must be finite";
        if (!(s->lo[k] < s->hi[k])) return "sv_voxel: the crop needs lo < hi on every axis";
        const double cells = ceil((s->hi[k] - s->lo[k]) / s->size);  // +inf where the difference or the quotient overflows
        if (!(cells <= 1048576.0)) return "sv_voxel: more than 2^20 cells on an axis";
        nc[k] = cells < 1.0 ? 1 : (int)cells;
    }
    return check_frame("sv_voxel", batch, width, height, 0);
}

const char *check_capacity(int capacity) {
    if (capacity < 1) return "sv_voxel: capacity < 1";
    if (capacity > MAX_CAPACITY) return "sv_voxel: capacity > 2^26";
    return nullptr;
}

int log2_slots(int capacity) {  // of a checked capacity: 10 .. 27
    const int64_t need = 2 * (int64_t)(capacity > sv::VOXEL_MIN_CAPACITY ? capacity : (int)sv::VOXEL_MIN_CAPACITY);
    int l = 10;
    while (((int64_t)1 << l) < need) l++;
    return l;
}

struct Layout {
    int Wv, n_visited, n_tiles, n_words, log2_slots;
    size_t mask_offset, pair_bytes, tiles_offset, total;
};

Layout layout(const sv_voxel_spec *s, int batch, int width, int height, int capacity) {
    Layout l;
    const int64_t wv = ((int64_t)width + s->step - 1) / s->step, hv = ((int64_t)height + s->step - 1) / s->step;
    l.Wv = (int)wv;
    l.n_visited = (int)(wv * hv);  // <= width * height < 2^31
    l.n_tiles = (int)((wv * hv + sv::CLOUD_TILE - 1) / sv::CLOUD_TILE);
    l.n_words = (int)((wv * hv + 31) / 32);
    l.log2_slots = log2_slots(capacity);
    l.mask_offset = ((size_t)1 << l.log2_slots) * sv::VOXEL_ENTRY_WORDS * 8 + sv::VOXEL_HEAD_BYTES;
    l.pair_bytes = l.mask_offset + ((size_t)l.n_words * 4 + 15) / 16 * 16;
    l.tiles_offset = (size_t)batch * l.pair_bytes;  // <= 2^16 * (2^27 * 72 + 2^28 + 32) < 2^50
    l.total = l.tiles_offset + (size_t)batch * l.n_tiles * sizeof(int32_t);
    return l;
}

enum { STAGE_CLEAR = 1, STAGE_INSERT, STAGE_MARK, STAGE_SCAN, STAGE_ALL };

int last_stage() {
    const char *e = getenv("SV_VOXEL_STAGE");
    if (!e) return STAGE_ALL;
    if (!strcmp(e, "clear")) return STAGE_CLEAR;
    if (!strcmp(e, "insert")) return STAGE_INSERT;
    if (!strcmp(e, "mark")) return STAGE_MARK;
    if (!strcmp(e, "scan")) return STAGE_SCAN;
    return STAGE_ALL;
}

}  // namespace

extern "C" {

int64_t sv_voxel_table_slots(int capacity) {
    if (check_capacity(capacity)) return -1;
    return (int64_t)1 << log2_slots(capacity);
}

size_t sv_voxel_workspace_bytes(const sv_voxel_spec *spec, int batch, int width, int height, int capacity) {
    int nc[3];
    if (check_shape(spec, batch, width, height, nc) || check_capacity(capacity)) return SIZE_MAX;
    return layout(spec, batch, width, height, capacity).total;
}

int sv_debug_voxel(int combine, unsigned long long *counters_device) {
    g_combine.store(combine != 0 ? 1 : 0);
    g_counters.store(counters_device);
    return SV_OK;
}

int sv_voxel_disparity_device(const float *disp, const uint8_t *colors, int batch, int width, int height, const double *Q16, const double *XR9,
                              const double *XT3, const sv_voxel_spec *spec, int capacity, void *xyz, uint8_t *color_out, int32_t *cell_out, int32_t *n_out,
                              int32_t *first_out, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream) {
    int nc[3];
    if (const char *bad = check_shape(spec, batch, width, height, nc)) return refuse(bad);
    if (const char *bad = check_capacity(capacity)) return refuse(bad);
    if (!disp) return refuse("sv_voxel: disp is NULL");
    if (!Q16) return refuse("sv_voxel: Q16 is NULL");
    if (!counts) return refuse("sv_voxel: counts is NULL");
    if (!xyz) return refuse("sv_voxel: xyz is NULL");
    if (color_out && !colors) return refuse("sv_voxel: color_out without colors");
    if ((reinterpret_cast<uintptr_t>(colors) | reinterpret_cast<uintptr_t>(color_out)) & 3) return refuse("sv_voxel: colors / color_out are not 4-byte aligned");
    const Layout l = layout(spec, batch, width, height, capacity);
    if (batch > 0 && (!workspace || workspace_bytes < l.total || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return refuse("sv_voxel: the workspace is NULL, not 16-byte aligned or smaller than sv_voxel_workspace_bytes");
    if (batch == 0) return SV_OK;

    sv::VoxelArgs a;
    memset(&a, 0, sizeof(a));
    set_reproject(a.c.rp, Q16, XR9, XT3);
    for (int k = 0; k < 3; k++) a.c.lo[k] = spec->lo[k], a.c.hi[k] = spec->hi[k], a.nc[k] = nc[k];
    a.size = spec->size;
    a.c.disp = disp, a.c.colors = color_out ? colors : nullptr;  // colours are summed only where they are asked for
    a.c.xyz = xyz, a.c.color_out = color_out, a.c.counts = counts;
    a.cell_out = cell_out, a.n_out = n_out, a.first_out = first_out;
    a.c.W = width, a.c.H = height, a.c.step = spec->step, a.c.capacity = capacity;
    a.c.Wv = l.Wv, a.c.n_visited = l.n_visited, a.c.n_tiles = l.n_tiles;
    a.n_words = l.n_words, a.log2_slots = l.log2_slots;
    a.ws = static_cast<uint8_t *>(workspace);
    a.pair_bytes = l.pair_bytes, a.mask_offset = l.mask_offset;
    a.c.tiles = reinterpret_cast<int32_t *>(a.ws + l.tiles_offset);
    a.counters = g_counters.load();

    hipStream_t st = static_cast<hipStream_t>(stream);
    const int last = last_stage();
    bool ok = sv::launch_voxel_clear(a, batch, st) == hipSuccess;
    if (ok && last >= STAGE_INSERT) ok = sv::launch_voxel_insert(spec->disparity, g_combine.load() != 0, a, batch, st) == hipSuccess;
    if (ok && last >= STAGE_MARK) ok = sv::launch_voxel_mark(a, batch, st) == hipSuccess;
    if (ok && last >= STAGE_SCAN) ok = sv::launch_voxel_count(a, batch, st) == hipSuccess && sv::launch_cloud_scan(a.c, batch, st) == hipSuccess;
    if (ok && last >= STAGE_ALL) ok = sv::launch_voxel_write(spec->disparity, spec->dtype, a, batch, st) == hipSuccess;
    if (!ok) {
        sv_internal_set_error("sv_voxel: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
