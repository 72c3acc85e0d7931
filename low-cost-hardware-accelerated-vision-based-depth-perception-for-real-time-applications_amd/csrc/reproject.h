// Per-pixel reprojection shared by k_reproject_batch (legacy_kernels.hip) and the fused top view (top_view_kernels.hip): one copy of
// the arithmetic, so the two produce the same doubles.  publishPointCloud (stereo_vision.cpp:233-256): pos = Q*[x y d 1]^T,
// (X,Y,Z) = pos.xyz / pos.w in double, then optionally the CUDA variant's robot-frame transform point = XR * (X, Y, Z) + XT
// (parallel_includes/main/stereo_vision.cu:188-212).  The build passes -ffp-contract=off: no FMA, the products and sums are rounded
// one by one in the order written, as numpy computes them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

// Q / XR / XT travel as kernel arguments.
struct ReprojectArgs {
    double Q[16], XR[9], XT[3];
    int has_xf;
};

#ifdef __HIP__  // the device functions; host code (top_view.cpp) only needs ReprojectArgs

// leftdpf.convertTo(dmap, CV_8UC1, 4.0) (stereo_vision.cpp:316): round half to even, saturate.
__device__ __forceinline__ int sv_dmap_u8(float d) {
    int v = __float2int_rn(d * 4.0f);
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ void sv_reproject_point(const ReprojectArgs &a, double x, double y, double d, double &X, double &Y, double &Z) {
    double pos[4];
#pragma unroll
    for (int r = 0; r < 4; r++) pos[r] = ((a.Q[4 * r] * x + a.Q[4 * r + 1] * y) + a.Q[4 * r + 2] * d) + a.Q[4 * r + 3];
    X = pos[0] / pos[3], Y = pos[1] / pos[3], Z = pos[2] / pos[3];
    if (a.has_xf) {
        const double px = ((a.XR[0] * X + a.XR[1] * Y) + a.XR[2] * Z) + a.XT[0];
        const double py = ((a.XR[3] * X + a.XR[4] * Y) + a.XR[5] * Z) + a.XT[1];
        const double pz = ((a.XR[6] * X + a.XR[7] * Y) + a.XR[8] * Z) + a.XT[2];
        X = px, Y = py, Z = pz;
    }
}

#endif

}  // namespace sv
