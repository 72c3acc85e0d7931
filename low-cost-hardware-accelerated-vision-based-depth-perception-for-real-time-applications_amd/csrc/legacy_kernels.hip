// Back-end maps of the legacy entry point, on the GPU (its front end - resize, gray conversion, remap -
// is the rig's, rig_kernels.hip):
//   f32 -> u8 x4        leftdpf.convertTo(dmap, CV_8UC1, 4.0) = saturate(round-half-even(4*d))       stereo_vision.cpp:316
//   reprojection        pos = Q*[i j d 1]^T, (X,Y,Z) = pos.xyz / pos.w in double                     :233-256
// OpenCV is an un-vendored dependency of the reference: these restate its documented arithmetic (parity unpinned).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reproject.h"

namespace sv {

__global__ __launch_bounds__(256) void k_dmap_cloud(const float *__restrict__ disp, uint8_t *__restrict__ dmap, double *__restrict__ pts, const double *__restrict__ Q, int W, int H) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= W) return;
    const size_t p = (size_t)j * W + i;
    int v = __float2int_rn(disp[p] * 4.0f);  // cvRound: round half to even
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    dmap[p] = (uint8_t)v;
    const double x = (double)i, y = (double)j, d = (double)v;
    double pos[4];
#pragma unroll
    for (int r = 0; r < 4; r++) pos[r] = ((Q[4 * r] * x + Q[4 * r + 1] * y) + Q[4 * r + 2] * d) + Q[4 * r + 3];
    pts[3 * p] = pos[0] / pos[3];
    pts[3 * p + 1] = pos[1] / pos[3];
    pts[3 * p + 2] = pos[2] / pos[3];
}

void launch_dmap_and_cloud(const float *disp, unsigned char *dmap, double *points, const double *Q16, int W, int H, hipStream_t st) {
    hipLaunchKernelGGL(k_dmap_cloud, dim3((W + 255) / 256, H), dim3(256), 0, st, disp, dmap, points, Q16, W, H);
}

// leftdpf.convertTo(dmap, CV_8UC1, 4.0) alone (stereo_vision.cpp:316), four pixels per thread: what a consumer that wants the driver's
// 8-bit disparity image - e.g. a gather of finished maps over xGMI, a quarter of the float maps' bytes - takes instead of D1.
__global__ __launch_bounds__(256) void k_disp_to_u8(const float *__restrict__ disp, uint8_t *__restrict__ out, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    auto cv8 = [](float d) -> uint32_t {
        int v = __float2int_rn(d * 4.0f);  // cvRound: round half to even; saturate_cast<uchar>
        return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    };
    if (i + 3 < n && ((reinterpret_cast<uintptr_t>(disp + i) & 15) == 0) && ((reinterpret_cast<uintptr_t>(out + i) & 3) == 0)) {
        const float4 d = *reinterpret_cast<const float4 *>(disp + i);
        *reinterpret_cast<uint32_t *>(out + i) = cv8(d.x) | (cv8(d.y) << 8) | (cv8(d.z) << 16) | (cv8(d.w) << 24);
    } else {
        for (size_t j = i; j < n && j < i + 4; j++) out[j] = (uint8_t)cv8(disp[j]);
    }
}

int launch_disp_to_u8(const float *disp, size_t n, unsigned char *out, hipStream_t st) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_disp_to_u8, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, st, disp, out, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Batched form with the CUDA variant's optional robot-frame transform (parallel_includes/main/stereo_vision.cu:188-212:
// point = XR * (X, Y, Z) + XT); the per-pixel arithmetic is reproject.h's, shared with the fused top view.
__global__ __launch_bounds__(256) void k_reproject_batch(const float *__restrict__ disp, uint8_t *__restrict__ dmap, double *__restrict__ pts, ReprojectArgs a, int W, int H) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= W) return;
    const size_t p = ((size_t)blockIdx.z * H + j) * W + i;
    const int v = sv_dmap_u8(disp[p]);
    if (dmap) dmap[p] = (uint8_t)v;
    double X, Y, Z;
    sv_reproject_point(a, (double)i, (double)j, (double)v, X, Y, Z);
    pts[3 * p] = X;
    pts[3 * p + 1] = Y;
    pts[3 * p + 2] = Z;
}

int launch_reproject_batch(const float *disp, int batch, int W, int H, const double *Q16, const double *XR9, const double *XT3, unsigned char *dmap, double *points,
                           hipStream_t st) {
    ReprojectArgs a;
    for (int i = 0; i < 16; i++) a.Q[i] = Q16[i];
    a.has_xf = (XR9 || XT3) ? 1 : 0;
    for (int i = 0; i < 9; i++) a.XR[i] = XR9 ? XR9[i] : (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; i++) a.XT[i] = XT3 ? XT3[i] : 0.0;
    hipLaunchKernelGGL(k_reproject_batch, dim3((W + 255) / 256, H, batch), dim3(256), 0, st, disp, dmap, points, a, W, H);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sv
