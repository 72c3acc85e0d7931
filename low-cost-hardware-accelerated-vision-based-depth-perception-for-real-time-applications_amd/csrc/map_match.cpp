// Group (L) of include/stereo_vision_hip.h: an occupancy frame matched against the world map over candidate poses (map_match_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "map_match_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_group{0};
std::atomic<unsigned long long *> g_lookups{nullptr};

// The three parts of the workspace, each a multiple of 16 bytes.
void layout(size_t cap, int batch, size_t *headers, size_t *partials, size_t *lists) {
    *headers = (size_t)batch * sizeof(sv::MapMatchHeader);
    *partials = (size_t)batch * sv::MAPMATCH_PARTIALS * sizeof(sv::MapMatchPartial);
    *lists = align16((size_t)batch * cap * sizeof(uint32_t));
}

}  // namespace

extern "C" {

int sv_map_match_workspace(const sv_occupancy_spec *frame, int batch, int w_free, size_t *bytes) {
    int frows, fcols;
    if (!frame || !bytes) return refuse("sv_map_match_workspace: the frame spec or bytes is NULL");
    if (sv_occupancy_dims(frame, &frows, &fcols) != SV_OK) return refuse("sv_map_match_workspace: the frame spec is not one sv_occupancy_dims admits");
    if (batch < 0 || batch > 65535) return refuse("sv_map_match_workspace: batch outside 0..65535");
    if (w_free < 0 || w_free > 32767) return refuse("sv_map_match_workspace: w_free outside 0..32767");
    size_t h, p, l;
    layout((size_t)frows * fcols, batch, &h, &p, &l);  // every cell may contribute, with or without the free ones
    *bytes = h + p + l;
    return SV_OK;
}

int sv_map_match_device(const uint8_t *state, const double *poses, int batch, int n_poses, const sv_occupancy_spec *frame, const sv_occupancy_map_spec *map,
                        const int16_t *logodds, int w_occ, int w_free, int64_t *sums, int32_t *counts, int32_t *best, int64_t *best_score, void *workspace,
                        size_t workspace_bytes, void *stream) {
    int frows, fcols;
    if (!frame) return refuse("sv_map_match: the frame spec is NULL");
    if (sv_occupancy_dims(frame, &frows, &fcols) != SV_OK) return refuse("sv_map_match: the frame spec is not one sv_occupancy_dims admits");
    if (const char *bad = check_map("sv_map_match", map)) return refuse(bad);
    if (batch < 0 || batch > 65535) return refuse("sv_map_match: batch outside 0..65535");
    if (n_poses < 1 || n_poses > 65535) return refuse("sv_map_match: n_poses outside 1..65535");
    if ((long long)batch * n_poses >= (1ll << 31)) return refuse("sv_map_match: batch x n_poses is 2^31 or more");
    if (w_occ < 0 || w_occ > 32767 || w_free < 0 || w_free > 32767) return refuse("sv_map_match: w_occ or w_free outside 0..32767");
    if (w_occ == 0 && w_free == 0) return refuse("sv_map_match: w_occ and w_free are both 0");
    if (!logodds) return refuse("sv_map_match: logodds is NULL");
    if ((sums == nullptr) != (counts == nullptr)) return refuse("sv_map_match: only one of sums and counts is given");
    if ((best == nullptr) != (best_score == nullptr)) return refuse("sv_map_match: only one of best and best_score is given");
    if (!sums && !best) return refuse("sv_map_match: neither sums and counts nor best and best_score are given");
    if (batch > 0 && (!state || !poses)) return refuse("sv_map_match: state or poses is NULL");
    size_t h, p, l;
    layout((size_t)frows * fcols, batch, &h, &p, &l);
    if (batch > 0 && !workspace) return refuse("sv_map_match: the workspace is NULL");
    if (workspace_bytes < h + p + l) return refuse("sv_map_match: the workspace is smaller than sv_map_match_workspace asks for");
    if (misaligned(poses, 8)) return refuse("sv_map_match: poses is not 8-byte aligned");
    if (misaligned(logodds, 2)) return refuse("sv_map_match: logodds is not 2-byte aligned");
    if (any_misaligned(8, sums, best_score)) return refuse("sv_map_match: sums or best_score is not 8-byte aligned");
    if (any_misaligned(4, counts, best)) return refuse("sv_map_match: counts or best is not 4-byte aligned");
    if (misaligned(workspace, 16)) return refuse("sv_map_match: the workspace is not 16-byte aligned");
    if (batch == 0) return SV_OK;  // nothing to do

    sv::MapMatchArgs a;
    memset(&a, 0, sizeof(a));
    a.state = state, a.poses = poses, a.logodds = logodds;
    a.sums = reinterpret_cast<long long *>(sums), a.counts = counts, a.best = best, a.best_score = reinterpret_cast<long long *>(best_score);
    char *ws = static_cast<char *>(workspace);
    a.headers = reinterpret_cast<sv::MapMatchHeader *>(ws);
    a.partials = reinterpret_cast<sv::MapMatchPartial *>(ws + h);
    a.lists = reinterpret_cast<uint32_t *>(ws + h + p);
    a.lookups = g_lookups.load();
    a.cap = (size_t)frows * fcols;
    a.B = batch, a.P = n_poses;
    a.frows = frows, a.fcols = fcols;
    a.m = sv::map_cells_of(*map);
    a.w_occ = w_occ, a.w_free = w_free;
    const double fs = (double)frame->scale;
    a.hf = 1.0 / (2.0 * fs);
    a.fr1 = trunc(frame->x_range[1] * fs), a.fc1 = trunc(frame->y_range[1] * fs);  // |.| <= 2^46: exact
    // candidates per workgroup: as many as still leave the chip about 1024 workgroups, or what the test hook asks for; never more
    // workgroups per frame than a frame has pairs for
    auto groups = [&](int g) { return (n_poses + (1 << g) - 1) >> g; };
    int g = 0;
    if (const int forced = g_group.load()) {
        while ((1 << g) < forced) g++;
    } else {
        for (int k = sv::MAPMATCH_MAX_LOG_GROUP; k > 0; k--)
            if ((long long)batch * groups(k) >= 1024) {
                g = k;
                break;
            }
    }
    while (groups(g) > sv::MAPMATCH_PARTIALS) g++;  // n_poses <= 65535: at most 2^5
    a.log_group = g, a.n_groups = groups(g);

    int stages = 3;
    if (const char *s = getenv("SV_MAP_MATCH_STAGE")) stages = !strcmp(s, "lists") ? 1 : !strcmp(s, "scores") ? 2 : 3;
    if (sv::launch_map_match(a, static_cast<hipStream_t>(stream), stages) != hipSuccess) {
        sv_internal_set_error("sv_map_match: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_map_match(int group, unsigned long long *lookups_device) {
    if (group != 0 && (group < 1 || group > 256 || (group & (group - 1)))) return refuse("sv_debug_map_match: group must be 0 or a power of two in 1..256");
    g_group.store(group);
    g_lookups.store(lookups_device);
    return SV_OK;
}

} /* extern "C" */
