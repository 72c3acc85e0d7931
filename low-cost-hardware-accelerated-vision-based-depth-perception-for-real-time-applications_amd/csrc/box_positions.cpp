// Group (E) of include/stereo_vision_hip.h: 3-D positions per detector box from disparity maps or point clouds (box_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "box_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

// NULL for a good call, else what is wrong with it.
const char *check(const sv_box_spec *s, bool points_entry, const void *src, const void *boxes, const void *pos, int batch, int width, int height, int max_boxes) {
    if (!s) return "sv_box_positions: spec is NULL";
    if (!src) return points_entry ? "sv_box_positions: points is NULL" : "sv_box_positions: disp is NULL";
    if (!boxes) return "sv_box_positions: boxes is NULL";
    if (!pos) return "sv_box_positions: pos is NULL";
    for (int k = 0; k < 5; k++)
        if (s->reserved[k] != 0) return "sv_box_positions: a reserved word of the spec is not 0";
    if (s->select != SV_BOX_ALL && s->select != SV_BOX_VALID && s->select != SV_BOX_NEAR) return "sv_box_positions: select is not SV_BOX_ALL / VALID / NEAR";
    if (s->disparity != SV_BOX_DMAP && s->disparity != SV_BOX_D1) return "sv_box_positions: disparity is not SV_BOX_DMAP / SV_BOX_D1";
    if (s->band < 0) return "sv_box_positions: band < 0";
    if (points_entry && s->select != SV_BOX_ALL) return "sv_box_positions: a point cloud has no disparity, only SV_BOX_ALL applies";
    if (batch < 0 || batch > 65535) return "sv_box_positions: batch outside 0..65535";
    if (max_boxes < 0 || max_boxes > 65535) return "sv_box_positions: max_boxes outside 0..65535";
    if (width < 1 || height < 1) return "sv_box_positions: width or height < 1";
    if ((int64_t)width * height >= ((int64_t)1 << 31)) return "sv_box_positions: width * height >= 2^31";
    return nullptr;
}

sv::BoxArgs base_args(const sv_box_spec *s, int width, int height, const int32_t *boxes, const int32_t *n_boxes, int max_boxes, double *pos, int32_t *stat) {
    sv::BoxArgs a;
    memset(&a, 0, sizeof(a));
    a.boxes = boxes, a.n_boxes = n_boxes;
    a.pos = pos, a.stat = stat;
    a.W = width, a.H = height, a.max_boxes = max_boxes, a.band = s->band;
    return a;
}

int launch(int src, const sv_box_spec *s, const sv::BoxArgs &a, int batch, void *stream) {
    if (sv::launch_box_positions(src, s->select, a, batch, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_box_positions: the kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

}  // namespace

extern "C" {

int sv_box_positions_disparity_device(const float *disp, int batch, int width, int height, const double *Q16, const double *XR9, const double *XT3,
                                      const int32_t *boxes, const int32_t *n_boxes, int max_boxes, const sv_box_spec *spec, double *pos, int32_t *stat,
                                      void *stream) {
    if (const char *bad = check(spec, false, disp, boxes, pos, batch, width, height, max_boxes)) return refuse(bad);
    if (!Q16) return refuse("sv_box_positions: Q16 is NULL");
    if (batch == 0 || max_boxes == 0) return SV_OK;
    sv::BoxArgs a = base_args(spec, width, height, boxes, n_boxes, max_boxes, pos, stat);
    set_reproject(a.rp, Q16, XR9, XT3);
    a.disp = disp;
    return launch(spec->disparity == SV_BOX_D1 ? sv::BOX_SRC_D1 : sv::BOX_SRC_DMAP, spec, a, batch, stream);
}

int sv_box_positions_points_device(const double *points, int batch, int width, int height, const int32_t *boxes, const int32_t *n_boxes, int max_boxes,
                                   const sv_box_spec *spec, double *pos, int32_t *stat, void *stream) {
    if (const char *bad = check(spec, true, points, boxes, pos, batch, width, height, max_boxes)) return refuse(bad);
    if (batch == 0 || max_boxes == 0) return SV_OK;
    sv::BoxArgs a = base_args(spec, width, height, boxes, n_boxes, max_boxes, pos, stat);
    a.points = points;
    return launch(sv::BOX_SRC_POINTS, spec, a, batch, stream);
}

} /* extern "C" */
