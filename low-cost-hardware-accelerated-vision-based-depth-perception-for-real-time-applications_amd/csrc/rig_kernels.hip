// Camera front end of a stereo rig (rig.cpp): B pairs of camera frames -> the engine's gray, matching-size, optionally
// rectified u8 images, both sides of the whole batch in one launch per pass.  The arithmetic is the OpenCV 4.x chain the
// reference-compatible entry restates (stereo_vision.cpp:338-341, 590-591), per output pixel and in this order:
//   1. cv::resize(INTER_LINEAR) per channel when the frame's size differs from the matching size: per destination column
//      fx = (float)((dx + 0.5) * scale_x - 0.5), sx = floor(fx), fx -= sx (clamped to the first / last source column with
//      fx = 0), 11-bit coefficients cvRound((1 - fx) * 2048), cvRound(fx * 2048); rows likewise, their indices clipped
//      instead; horizontal blend in int, vertical ((b0*(h0>>4))>>16) + ((b1*(h1>>4))>>16) + 2) >> 2.  Exact 2x decimation in
//      both directions takes OpenCV's INTER_AREA shortcut (sum of the 2x2 block + 2) >> 2.
//   2. cv::cvtColor(BGR[A]2GRAY): 15-bit weights B 3735, G 19235, R 9798, (+16384) >> 15.  A gray source passes unchanged.
//   3. cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) when rectification is on: map coordinates cvRound(map * 32) (done once per
//      rig on the host, rig.cpp), 5 fractional bits, weights (32-fx)(32-fy)*32 ... summing to 2^15, (sum + 2^14) >> 15.
// Passes: without resize one pass (gray, or gray and remap fused: every remap tap is converted as it is read); with resize
// resize+gray in one pass and, with rectification, the remap of the gray image in a second.
//
// Layout: one lane = 4 consecutive output pixels of one row (a 16-B load of 4 BGRA pixels, 12 B for BGR / RGB, 4 B for gray,
// scalar loads where a row's address is not a multiple of 4; one dword store of the 4 gray pixels).  Blocks of 256 lanes
// cover 1024 output pixels of one image; the 1-D grid runs the batch fastest (block = (tile, side, pair)), so the pairs of a
// batch read the same tile of their side's map back to back while it is in L2 / the Infinity Cache.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rig_kernels.h"

namespace sv {

namespace {

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
struct u32x3_a4 {
    uint32_t a, b, c;
};

template <int F>
__device__ constexpr int channels() {
    return F == RIG_PIX_BGRA ? 4 : (F == RIG_PIX_GRAY ? 1 : 3);
}

__device__ __forceinline__ uint32_t from_rgb(uint32_t t) {  // R | G << 8 | B << 16 -> B | G << 8 | R << 16 | 255 << 24
    return ((t & 0xffu) << 16) | (t & 0xff00u) | ((t >> 16) & 0xffu) | 0xff000000u;
}

// one source pixel as B | G << 8 | R << 16 | A << 24 (A = 255 for 3-channel and gray sources)
template <int F>
__device__ __forceinline__ uint32_t load_px(const uint8_t *p) {
    if (F == RIG_PIX_BGRA) {
        if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const uint32_t *>(p);
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    if (F == RIG_PIX_BGR) return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | 0xff000000u;
    if (F == RIG_PIX_RGB) return (uint32_t)p[2] | ((uint32_t)p[1] << 8) | ((uint32_t)p[0] << 16) | 0xff000000u;
    return (uint32_t)p[0] * 0x010101u | 0xff000000u;
}

__device__ __forceinline__ uint32_t gray_of(uint32_t bgra) {
    return ((bgra & 255u) * 3735u + ((bgra >> 8) & 255u) * 19235u + ((bgra >> 16) & 255u) * 9798u + 16384u) >> 15;
}

// pixels x0 .. x0+n-1 of a source row
template <int F>
__device__ __forceinline__ void load4(const uint8_t *row, int x0, int n, uint32_t px[4]) {
    constexpr int C = channels<F>();
    const uint8_t *p = row + (size_t)x0 * C;
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        if (F == RIG_PIX_BGRA) {
            const u32x4_a4 v = *reinterpret_cast<const u32x4_a4 *>(p);
            px[0] = v.x, px[1] = v.y, px[2] = v.z, px[3] = v.w;
        } else if (F == RIG_PIX_GRAY) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
            for (int i = 0; i < 4; i++) px[i] = ((w >> (8 * i)) & 255u) * 0x010101u | 0xff000000u;
        } else {  // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            const u32x3_a4 v = *reinterpret_cast<const u32x3_a4 *>(p);
            const uint32_t t0 = v.a & 0xffffffu, t1 = (v.a >> 24) | ((v.b & 0xffffu) << 8), t2 = (v.b >> 16) | ((v.c & 0xffu) << 16), t3 = v.c >> 8;
            if (F == RIG_PIX_BGR) {
                px[0] = t0 | 0xff000000u, px[1] = t1 | 0xff000000u, px[2] = t2 | 0xff000000u, px[3] = t3 | 0xff000000u;
            } else {
                px[0] = from_rgb(t0), px[1] = from_rgb(t1), px[2] = from_rgb(t2), px[3] = from_rgb(t3);
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) px[i] = i < n ? load_px<F>(p + i * C) : 0u;
}

__device__ __forceinline__ void store_gray4(uint8_t *o, int n, const uint32_t g[4]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(o);
    if (n == 4 && (a & 3) == 0) {
        *reinterpret_cast<uint32_t *>(o) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
    } else if (n == 4 && (a & 1) == 0) {
        reinterpret_cast<uint16_t *>(o)[0] = (uint16_t)(g[0] | (g[1] << 8));
        reinterpret_cast<uint16_t *>(o)[1] = (uint16_t)(g[2] | (g[3] << 8));
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < n) o[i] = (uint8_t)g[i];
    }
}

__device__ __forceinline__ void store_bgra4(uint8_t *o, int n, const uint32_t px[4]) {  // o: 4-byte aligned (checked by the caller of the ABI)
    if (n == 4) {
        *reinterpret_cast<u32x4_a4 *>(o) = u32x4_a4{px[0], px[1], px[2], px[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < n) reinterpret_cast<uint32_t *>(o)[i] = px[i];
    }
}

// block -> (side, pair, row, first column, pixel count); false for the lanes past the image's last group
__device__ __forceinline__ bool locate(const RigArgs &a, int &side, int &b, int &y, int &x0, int &n) {
    const int pairs2 = 2 * a.batch;
    const int j = (int)(blockIdx.x % (unsigned)pairs2), tile = (int)(blockIdx.x / (unsigned)pairs2);
    side = j >= a.batch ? 1 : 0;
    b = j - side * a.batch;
    const int gid = tile * 256 + (int)threadIdx.x;
    if (gid >= a.groups * a.H) return false;
    y = gid / a.groups;
    x0 = (gid - y * a.groups) * 4;
    n = min(4, a.W - x0);
    return true;
}

// bilinear fixed-point remap of one output pixel; the taps are gray values of a W x H image read through load_px
template <int F>
__device__ __forceinline__ uint32_t remap_px(const uint8_t *img, size_t pitch, int W, int H, int2 q) {
    constexpr int C = channels<F>();
    const int ix = q.x >> 5, iy = q.y >> 5, fx = q.x & 31, fy = q.y & 31;
    auto at = [&](int x, int y) -> int {
        return (x >= 0 && x < W && y >= 0 && y < H) ? (int)gray_of(load_px<F>(img + (size_t)y * pitch + (size_t)x * C)) : 0;
    };
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const int v = at(ix, iy) * w00 + at(ix + 1, iy) * w01 + at(ix, iy + 1) * w10 + at(ix + 1, iy + 1) * w11;
    return (uint32_t)((v + (1 << 14)) >> 15);
}

// no resize: gray (REMAP = false) or gray + remap fused; optional colours of the left image
template <int F, bool REMAP>
__global__ __launch_bounds__(256) void k_rig_direct(RigArgs a) {
    int side, b, y, x0, n;
    if (!locate(a, side, b, y, x0, n)) return;
    const uint8_t *img = a.src[side] + (size_t)b * a.src_frame;
    const size_t o = ((size_t)b * a.H + y) * a.W + x0;
    uint32_t g[4], px[4];
    const bool colours = side == 0 && a.colours != nullptr;
    if (!REMAP || colours) load4<F>(img + (size_t)y * a.pitch, x0, n, px);
    if (REMAP) {
        const int2 *m = a.maps[side] + (size_t)y * a.W + x0;
        int2 q[4];
        if (n == 4) {
            const u32x4_a4 m01 = reinterpret_cast<const u32x4_a4 *>(m)[0], m23 = reinterpret_cast<const u32x4_a4 *>(m)[1];
            q[0] = make_int2((int)m01.x, (int)m01.y), q[1] = make_int2((int)m01.z, (int)m01.w);
            q[2] = make_int2((int)m23.x, (int)m23.y), q[3] = make_int2((int)m23.z, (int)m23.w);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] = i < n ? m[i] : make_int2(0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = i < n ? remap_px<F>(img, a.pitch, a.W, a.H, q[i]) : 0u;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = gray_of(px[i]);
    }
    store_gray4(a.dst[side] + o, n, g);
    if (colours) store_bgra4(a.colours + 4 * o, n, px);
}

// resize + gray (into the output, or into the intermediate of the remap pass); optional colours of the left image
template <int F>
__global__ __launch_bounds__(256) void k_rig_resize(RigArgs a) {
    constexpr int C = channels<F>();
    int side, b, y, x0, n;
    if (!locate(a, side, b, y, x0, n)) return;
    const uint8_t *img = a.src[side] + (size_t)b * a.src_frame;
    const size_t o = ((size_t)b * a.H + y) * a.W + x0;
    uint32_t px[4];
    if (a.area2) {
        const uint8_t *r0 = img + (size_t)(2 * y) * a.pitch, *r1 = r0 + a.pitch;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i >= n) {
                px[i] = 0;
                continue;
            }
            const int sx = 2 * (x0 + i);
            const uint32_t p00 = load_px<F>(r0 + (size_t)sx * C), p01 = load_px<F>(r0 + (size_t)(sx + 1) * C);
            const uint32_t p10 = load_px<F>(r1 + (size_t)sx * C), p11 = load_px<F>(r1 + (size_t)(sx + 1) * C);
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int s = 8 * c;
                v |= ((((p00 >> s) & 255u) + ((p01 >> s) & 255u) + ((p10 >> s) & 255u) + ((p11 >> s) & 255u) + 2u) >> 2) << s;
            }
            px[i] = v;
        }
    } else {
        float fy = (float)(((double)y + 0.5) * a.scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int b0 = __float2int_rn((1.f - fy) * 2048.f), b1 = __float2int_rn(fy * 2048.f);
        const int y0 = min(max(sy, 0), a.sh - 1), y1 = min(max(sy + 1, 0), a.sh - 1);
        const uint8_t *r0 = img + (size_t)y0 * a.pitch, *r1 = img + (size_t)y1 * a.pitch;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i >= n) {
                px[i] = 0;
                continue;
            }
            float fx = (float)(((double)(x0 + i) + 0.5) * a.scale_x - 0.5);
            int sx = (int)floorf(fx);
            fx -= (float)sx;
            if (sx < 0) fx = 0.f, sx = 0;
            if (sx >= a.sw - 1) fx = 0.f, sx = a.sw - 1;
            const int a0 = __float2int_rn((1.f - fx) * 2048.f), a1 = __float2int_rn(fx * 2048.f);
            const int sx1 = min(sx + 1, a.sw - 1);
            const uint32_t p00 = load_px<F>(r0 + (size_t)sx * C), p01 = load_px<F>(r0 + (size_t)sx1 * C);
            const uint32_t p10 = load_px<F>(r1 + (size_t)sx * C), p11 = load_px<F>(r1 + (size_t)sx1 * C);
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int s = 8 * c;
                const int h0 = (int)((p00 >> s) & 255u) * a0 + (int)((p01 >> s) & 255u) * a1;
                const int h1 = (int)((p10 >> s) & 255u) * a0 + (int)((p11 >> s) & 255u) * a1;
                v |= (uint32_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2) << s;
            }
            px[i] = v;
        }
    }
    uint32_t g[4];
#pragma unroll
    for (int i = 0; i < 4; i++) g[i] = gray_of(px[i]);
    store_gray4(a.dst[side] + o, n, g);
    if (side == 0 && a.colours) store_bgra4(a.colours + 4 * o, n, px);
}

// remap of a gray W x H intermediate (second pass after a resize)
__global__ __launch_bounds__(256) void k_rig_remap(RigArgs a) {
    int side, b, y, x0, n;
    if (!locate(a, side, b, y, x0, n)) return;
    const uint8_t *img = a.src[side] + (size_t)b * a.src_frame;
    const int2 *m = a.maps[side] + (size_t)y * a.W + x0;
    uint32_t g[4];
#pragma unroll
    for (int i = 0; i < 4; i++) g[i] = i < n ? remap_px<RIG_PIX_GRAY>(img, a.pitch, a.W, a.H, m[i]) : 0u;
    store_gray4(a.dst[side] + ((size_t)b * a.H + y) * a.W + x0, n, g);
}

template <int F>
hipError_t launch_format(RigPass pass, const RigArgs &a, dim3 grid, hipStream_t st) {
    switch (pass) {
    case RIG_PASS_GRAY: hipLaunchKernelGGL((k_rig_direct<F, false>), grid, dim3(256), 0, st, a); break;
    case RIG_PASS_GRAY_REMAP: hipLaunchKernelGGL((k_rig_direct<F, true>), grid, dim3(256), 0, st, a); break;
    case RIG_PASS_RESIZE_GRAY: hipLaunchKernelGGL((k_rig_resize<F>), grid, dim3(256), 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

int rig_grid_blocks(int W, int H, int batch, unsigned *blocks) {
    const size_t groups = ((size_t)W + 3) / 4, tiles = (groups * H + 255) / 256, n = tiles * 2 * (size_t)batch;
    if (n == 0 || n > 0x7fffffffu) return -1;
    *blocks = (unsigned)n;
    return 0;
}

hipError_t launch_rig_pass(RigPass pass, int format, const RigArgs &args, hipStream_t st) {
    RigArgs a = args;
    a.groups = (a.W + 3) / 4;
    unsigned blocks;
    if (rig_grid_blocks(a.W, a.H, a.batch, &blocks) != 0) return hipErrorInvalidValue;
    const dim3 grid(blocks);
    if (pass == RIG_PASS_REMAP) {
        hipLaunchKernelGGL(k_rig_remap, grid, dim3(256), 0, st, a);
        return hipGetLastError();
    }
    switch (format) {
    case RIG_PIX_BGRA: return launch_format<RIG_PIX_BGRA>(pass, a, grid, st);
    case RIG_PIX_BGR: return launch_format<RIG_PIX_BGR>(pass, a, grid, st);
    case RIG_PIX_RGB: return launch_format<RIG_PIX_RGB>(pass, a, grid, st);
    case RIG_PIX_GRAY: return launch_format<RIG_PIX_GRAY>(pass, a, grid, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace sv
