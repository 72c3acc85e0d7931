// Group (AD) of include/stereo_vision_hip.h: the voxels of one voxel map of (Q) moved by per-frame rigid corrections into another
// (voxel_repose_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and
// a refused call leaves its text for sv_last_error(NULL).  The check of a map's spec and buffer is stage_glue.h's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_repose_kernels.h"

namespace {

using namespace sv::glue;

constexpr int MAX_CORR = 1 << 22;         // corrections per call
constexpr int MAX_SEQ = 2147483646;       // the largest sequence number of a frame: 2^31 - 2

}  // namespace

extern "C" {

int sv_voxel_repose_device(void *dst, size_t dst_bytes, const sv_voxel_map_spec *dst_spec, const void *src, size_t src_bytes, const sv_voxel_map_spec *src_spec,
                           const double *corr, int n_corr, int seq0, int64_t min_n, int64_t min_rows, int since, int64_t *stats, void *stream) {
    int dst_nc[3], src_nc[3], dst_l, src_l;
    if (const char *bad = check_voxel_map("sv_voxel_repose: dst", dst, dst_bytes, dst_spec, dst_nc, &dst_l)) return refuse(bad);
    if (const char *bad = check_voxel_map("sv_voxel_repose: src", src, src_bytes, src_spec, src_nc, &src_l)) return refuse(bad);
    if (!corr) return refuse("sv_voxel_repose: corr is NULL");
    if (n_corr < 1 || n_corr > MAX_CORR) return refuse("sv_voxel_repose: n_corr outside 1 .. 2^22");
    if (seq0 < 0 || seq0 > MAX_SEQ) return refuse("sv_voxel_repose: seq0 outside 0 .. 2^31 - 2");
    if (misaligned(corr, 8)) return refuse("sv_voxel_repose: corr is not 8-byte aligned");
    if (overlap(dst, dst_bytes, src, src_bytes)) return refuse("sv_voxel_repose: the two maps overlap");
    const size_t corr_bytes = (size_t)n_corr * 12 * sizeof(double);
    if (overlap(corr, corr_bytes, dst, dst_bytes)) return refuse("sv_voxel_repose: corr lies inside dst");
    if (misaligned(stats, 8)) return refuse("sv_voxel_repose: stats is not 8-byte aligned");
    const size_t stats_bytes = sv::VREPOSE_STATS * sizeof(int64_t);
    if (overlap(stats, stats_bytes, dst, dst_bytes) || overlap(stats, stats_bytes, src, src_bytes)) return refuse("sv_voxel_repose: stats lies inside a map");
    if (overlap(stats, stats_bytes, corr, corr_bytes)) return refuse("sv_voxel_repose: stats lies inside corr");

    sv::VoxelReposeArgs a;
    memset(&a, 0, sizeof(a));
    a.dst = static_cast<uint8_t *>(dst), a.src = static_cast<const uint8_t *>(src);
    a.dst_log2_slots = dst_l, a.src_log2_slots = src_l, a.dst_capacity = dst_spec->capacity;
    for (int k = 0; k < 3; k++) a.lo[k] = dst_spec->lo[k], a.hi[k] = dst_spec->hi[k], a.nc[k] = dst_nc[k], a.src_lo[k] = src_spec->lo[k];
    a.size = dst_spec->size, a.src_size = src_spec->size;
    a.corr = corr, a.n_corr = n_corr, a.seq0 = seq0;
    a.min_n = min_n, a.min_rows = min_rows, a.since = since;
    a.stats = reinterpret_cast<long long *>(stats);
    if (sv::launch_voxel_repose(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_repose: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
