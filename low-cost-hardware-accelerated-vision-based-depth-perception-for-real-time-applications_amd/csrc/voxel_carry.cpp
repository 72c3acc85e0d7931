// Group (S) of include/stereo_vision_hip.h: the voxels of one voxel map of (Q) carried into another (voxel_carry_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).  The check of a map's spec and buffer is stage_glue.h's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_carry_kernels.h"

namespace {

using namespace sv::glue;

constexpr int MAX_SHIFT = 1 << 20;  // cells: an axis has at most that many, so a larger shift carries nothing either

}  // namespace

extern "C" {

int sv_voxel_map_carry_device(void *dst, size_t dst_bytes, const sv_voxel_map_spec *dst_spec, const void *src, size_t src_bytes, const sv_voxel_map_spec *src_spec,
                              int shift_x, int shift_y, int shift_z, int64_t min_n, int64_t min_rows, int since, int64_t *stats, void *stream) {
    int dst_nc[3], src_nc[3], dst_l, src_l;
    if (const char *bad = check_voxel_map("sv_voxel_map_carry: dst", dst, dst_bytes, dst_spec, dst_nc, &dst_l)) return refuse(bad);
    if (const char *bad = check_voxel_map("sv_voxel_map_carry: src", src, src_bytes, src_spec, src_nc, &src_l)) return refuse(bad);
    if (memcmp(&dst_spec->size, &src_spec->size, sizeof(double)) != 0) return refuse("sv_voxel_map_carry: the two maps differ in size");
    const int shift[3] = {shift_x, shift_y, shift_z};
    for (int k = 0; k < 3; k++)
        if (shift[k] < -MAX_SHIFT || shift[k] > MAX_SHIFT) return refuse("sv_voxel_map_carry: a shift outside -2^20 .. 2^20");
    if (overlap(dst, dst_bytes, src, src_bytes)) return refuse("sv_voxel_map_carry: the two maps overlap");
    if (misaligned(stats, 8)) return refuse("sv_voxel_map_carry: stats is not 8-byte aligned");
    const size_t stats_bytes = sv::VCARRY_STATS * sizeof(int64_t);
    if (overlap(stats, stats_bytes, dst, dst_bytes) || overlap(stats, stats_bytes, src, src_bytes)) return refuse("sv_voxel_map_carry: stats lies inside a map");

    sv::VoxelCarryArgs a;
    memset(&a, 0, sizeof(a));
    a.dst = static_cast<uint8_t *>(dst), a.src = static_cast<const uint8_t *>(src);
    a.dst_log2_slots = dst_l, a.src_log2_slots = src_l, a.dst_capacity = dst_spec->capacity;
    for (int k = 0; k < 3; k++) a.dst_nc[k] = dst_nc[k], a.shift[k] = shift[k];
    a.min_n = min_n, a.min_rows = min_rows, a.since = since;
    a.stats = reinterpret_cast<long long *>(stats);
    if (sv::launch_voxel_carry(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_map_carry: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
