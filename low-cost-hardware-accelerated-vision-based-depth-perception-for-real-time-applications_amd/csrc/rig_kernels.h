// Launch interface of rig_kernels.hip (the camera front end of rig.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

enum { RIG_PIX_BGRA = 0, RIG_PIX_BGR = 1, RIG_PIX_RGB = 2, RIG_PIX_GRAY = 3 };  // == sv_pixel_format

enum RigPass {
    RIG_PASS_GRAY = 0,         // source of the matching size -> gray
    RIG_PASS_GRAY_REMAP = 1,   // source of the matching size -> gray, remapped (fused)
    RIG_PASS_RESIZE_GRAY = 2,  // source of another size -> resized gray
    RIG_PASS_REMAP = 3,        // gray of the matching size -> remapped gray (after RIG_PASS_RESIZE_GRAY)
};

struct RigArgs {
    const uint8_t *src[2];  // left / right: B frames back to back, src_frame bytes apart, rows `pitch` bytes apart
    uint8_t *dst[2];        // left / right gray [B][H][W]
    uint8_t *colours;       // left image as BGRA [B][H][W][4] (before the remap), 4-byte aligned; NULL = not wanted
    const int2 *maps[2];    // left / right (cvRound(mapx * 32), cvRound(mapy * 32)) [H][W]; remap passes only
    size_t src_frame, pitch;
    int sw, sh;             // source size
    int W, H;               // matching size
    int batch;
    int groups;             // (W + 3) / 4, set by the launcher
    double scale_x, scale_y;  // sw / W, sh / H as cv::resize computes them (1 / inv_scale)
    int area2;              // sw == 2 W and sh == 2 H: the INTER_AREA shortcut
};

// Blocks of the 1-D grid of a pass (-1 if it does not fit a launch).
int rig_grid_blocks(int W, int H, int batch, unsigned *blocks);
hipError_t launch_rig_pass(RigPass pass, int format, const RigArgs &args, hipStream_t st);

}  // namespace sv
