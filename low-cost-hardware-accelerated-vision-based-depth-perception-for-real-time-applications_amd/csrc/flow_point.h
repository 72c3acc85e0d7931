// The device functions that groups (Z) and (AA) of include/stereo_vision_hip.h share (flow_kernels.hip, warp_kernels.hip): a disparity
// in 1/16 px, and a pixel's point moved by a pose.  Doubles in the definition's order, one operation at a time - the build contracts
// nothing -, so every kernel that includes this gives the bits of stereo_vision/sv.py's _flow_dq, _flow_point and _flow_move.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "flow_kernels.h"

namespace sv {

constexpr double FLOW_Z_MIN = 0.1, FLOW_CENTRE_MAX = 1048576.0;

// floor(16 d + 0.5) of a disparity that makes a point, else 0
__device__ __forceinline__ int flow_dq(float d) {
    if (!(d > 0.0f) || !isfinite(d)) return 0;
    const double q = floor((double)d * 16.0 + 0.5);
    return q >= 1.0 && q <= (double)FLOW_DQ_MAX ? (int)q : 0;
}

// X0 of pixel (u, v) with disparity dq / 16, then Xc under the pose's twelve doubles, in the definition's order
__device__ __forceinline__ void flow_point(const FlowCamera &c, const double *pose, int u, int v, int dq, double &x, double &y, double &z) {
    const double d = (double)dq;
    const double x0 = (((double)u - c.cx) * c.b16) / d, y0 = (((double)v - c.cy) * c.b16) / d, z0 = c.fb16 / d;
    x = ((pose[0] * x0 + pose[1] * y0) + pose[2] * z0) + pose[9];
    y = ((pose[3] * x0 + pose[4] * y0) + pose[5] * z0) + pose[10];
    z = ((pose[6] * x0 + pose[7] * y0) + pose[8] * z0) + pose[11];
}

}  // namespace sv
