// Group (C) of include/stereo_vision_hip.h: a calibrated stereo rig as a handle.  sv_rig_create reads the calibration and
// computes Q and the rectification maps on the host (stereoRectify / initUndistortRectifyMap restated in calib.cpp); the
// first device call uploads the maps, rounded once to the remap's fixed point; sv_rig_frontend_device turns a batch of
// camera frames into the engine's input with the kernels of rig_kernels.hip.  Nothing here is process-global except the
// error text of the last failed create (per thread, like sv_last_error(NULL)).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "calib.h"
#include "rig_kernels.h"

struct sv_rig {
    sv_rig_config cfg;
    sv::Calibration calib;
    sv::Rectification rect;
    std::vector<float> maps;      // [4][H][W] lmapx lmapy rmapx rmapy (rectify only)
    std::vector<int32_t> fixed;   // [2][H][W][2] (cvRound(mapx * 32), cvRound(mapy * 32)) per side
    int32_t *d_fixed = nullptr;   // device copy, made by the first device call
    std::mutex mu;
    std::string error;
};

namespace {

thread_local std::string g_rig_create_error;

int fail(std::string &where, int code, const std::string &msg) {
    where = msg;
    return code;
}

// cvRound(m * 32) as v_cvt_i32_f32 rounds it on the device (ties to even, NaN -> 0).  Values beyond +-2^30 are clamped: any
// coordinate that far outside the image puts all four taps outside it, exactly like the saturated conversion.
int32_t fixed5(float m) {
    const float v = m * 32.0f;
    if (v != v) return 0;
    if (v >= 1073741824.0f) return 1 << 30;
    if (v <= -1073741824.0f) return -(1 << 30);
    return (int32_t)lrintf(v);
}

int channels(int format) { return format == SV_PIX_BGRA8 ? 4 : (format == SV_PIX_GRAY8 ? 1 : 3); }

}  // namespace

extern "C" {

int sv_rig_create(const char *calibration_yaml, const sv_rig_config *cfg, sv_rig **out) {
    std::string &err = g_rig_create_error;
    char b[256];
    if (!out) return fail(err, SV_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!cfg) return fail(err, SV_ERR_ARG, "cfg is NULL");
    if (cfg->width < 32 || cfg->height < 32 || cfg->width > 8192 || cfg->height > 4096) {
        snprintf(b, sizeof(b), "unsupported matching size %dx%d (32..8192 x 32..4096)", cfg->width, cfg->height);
        return fail(err, SV_ERR_ARG, b);
    }
    if (!(cfg->scale > 0.0f) || !isfinite(cfg->scale)) return fail(err, SV_ERR_ARG, "scale must be a finite number > 0");
    if (cfg->rectify != 0 && cfg->rectify != 1) return fail(err, SV_ERR_ARG, "rectify must be 0 or 1");
    if (cfg->device < 0) return fail(err, SV_ERR_ARG, "device must be >= 0");
    for (int i = 0; i < 3; i++)
        if (cfg->reserved[i] != 0) return fail(err, SV_ERR_ARG, "sv_rig_config.reserved must be zero");
    if (!calibration_yaml) return fail(err, SV_ERR_ARG, "calibration file is NULL");
    sv_rig *r = new sv_rig();
    r->cfg = *cfg;
    std::string e;
    if (!sv::load_calibration_yaml(calibration_yaml, r->calib, e)) {
        delete r;
        return fail(err, SV_ERR_ARG, e);
    }
    for (int i = 0; i < 6; i++) {  // K1, K2 first two rows /= scale_factor (stereo_vision.cpp:364-376)
        r->calib.K1[i] /= cfg->scale;
        r->calib.K2[i] /= cfg->scale;
    }
    const int W = cfg->width, H = cfg->height;
    sv::stereo_rectify(r->calib, W, H, W, H, 0.0, r->rect);  // :439, calib_img_size == out_img_size (:524-525)
    if (cfg->rectify) {  // findRectificationMap's two initUndistortRectifyMap calls (stereo_vision.cpp:477-478)
        const size_t N = (size_t)W * H;
        r->maps.assign(4 * N, 0.f);
        float *m = r->maps.data();
        if (!sv::init_undistort_rectify_map(r->calib.K1, r->calib.D1, r->rect.R1, r->rect.P1, W, H, m, m + N) ||
            !sv::init_undistort_rectify_map(r->calib.K2, r->calib.D2, r->rect.R2, r->rect.P2, W, H, m + 2 * N, m + 3 * N)) {
            delete r;
            return fail(err, SV_ERR_ARG, "singular rectification");
        }
        r->fixed.resize(4 * N);
        for (int s = 0; s < 2; s++)
            for (size_t p = 0; p < N; p++) {
                r->fixed[2 * (s * N + p)] = fixed5(m[(2 * s) * N + p]);
                r->fixed[2 * (s * N + p) + 1] = fixed5(m[(2 * s + 1) * N + p]);
            }
    }
    *out = r;
    return SV_OK;
}

int sv_rig_destroy(sv_rig *r) {
    if (!r) return SV_ERR_ARG;
    if (r->d_fixed) {
        int prev = 0;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(r->cfg.device);
        (void)hipFree(r->d_fixed);  // synchronises with work still reading the maps
        (void)hipSetDevice(prev);
    }
    delete r;
    return SV_OK;
}

const char *sv_rig_last_error(const sv_rig *r) { return r ? r->error.c_str() : g_rig_create_error.c_str(); }

int sv_rig_matrices(const sv_rig *r, double *Q16, double *XR9, double *XT3) {
    if (!r) return SV_ERR_ARG;
    if (Q16) memcpy(Q16, r->rect.Q, sizeof(r->rect.Q));
    if (XR9 && r->calib.has_xr) memcpy(XR9, r->calib.XR, sizeof(r->calib.XR));
    if (XT3 && r->calib.has_xt) memcpy(XT3, r->calib.XT, sizeof(r->calib.XT));
    return (r->calib.has_xr ? 1 : 0) | (r->calib.has_xt ? 2 : 0);
}

int sv_rig_maps(const sv_rig *r, float *maps) {
    if (!r || !maps) return SV_ERR_ARG;
    if (!r->cfg.rectify) return SV_ERR_STATE;
    memcpy(maps, r->maps.data(), r->maps.size() * sizeof(float));
    return SV_OK;
}

int sv_rig_frontend_device(sv_rig *r, const uint8_t *left, const uint8_t *right, int batch, int src_width, int src_height, int src_pitch, int pixel_format,
                           uint8_t *gray_left, uint8_t *gray_right, uint8_t *left_bgra, void *stream) {
    if (!r) return SV_ERR_ARG;
    std::lock_guard<std::mutex> lk(r->mu);
    std::string &err = r->error;
    char b[256];
    if (pixel_format < SV_PIX_BGRA8 || pixel_format > SV_PIX_GRAY8) return fail(err, SV_ERR_ARG, "unknown pixel format");
    if (batch < 0) return fail(err, SV_ERR_ARG, "batch must be >= 0");
    if (src_width < 1 || src_height < 1 || (size_t)src_width * src_height > ((size_t)1 << 26)) {
        snprintf(b, sizeof(b), "bad source size %dx%d (at most 2^26 pixels)", src_width, src_height);
        return fail(err, SV_ERR_ARG, b);
    }
    if ((int64_t)src_pitch < (int64_t)src_width * channels(pixel_format)) return fail(err, SV_ERR_ARG, "src_pitch is smaller than a row");
    if (batch == 0) return SV_OK;
    if (!left || !right || !gray_left || !gray_right) return fail(err, SV_ERR_ARG, "NULL image pointer");
    if (reinterpret_cast<uintptr_t>(left_bgra) & 3) return fail(err, SV_ERR_ARG, "left_bgra must be 4-byte aligned");
    const int W = r->cfg.width, H = r->cfg.height;
    unsigned blocks;
    if (sv::rig_grid_blocks(W, H, batch, &blocks) != 0) return fail(err, SV_ERR_ARG, "batch too large for one launch");
    const bool resize = src_width != W || src_height != H;
    const bool remap = r->cfg.rectify != 0;

    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess) return fail(err, SV_ERR_NO_DEVICE, "no HIP device");
    struct Restore {
        int d;
        ~Restore() { (void)hipSetDevice(d); }
    } restore{prev};
    hipError_t e = hipSetDevice(r->cfg.device);
    if (e != hipSuccess) return fail(err, SV_ERR_NO_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)W * H;
    if (remap && !r->d_fixed) {
        if ((e = hipMalloc((void **)&r->d_fixed, r->fixed.size() * sizeof(int32_t))) != hipSuccess ||
            (e = hipMemcpy(r->d_fixed, r->fixed.data(), r->fixed.size() * sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess) {
            if (r->d_fixed) (void)hipFree(r->d_fixed);
            r->d_fixed = nullptr;
            return fail(err, SV_ERR_HIP, std::string("rectification maps: ") + hipGetErrorString(e));
        }
    }
    sv::RigArgs a;
    memset(&a, 0, sizeof(a));
    a.src[0] = left;
    a.src[1] = right;
    a.dst[0] = gray_left;
    a.dst[1] = gray_right;
    a.colours = left_bgra;
    if (remap) {
        a.maps[0] = reinterpret_cast<const int2 *>(r->d_fixed);
        a.maps[1] = reinterpret_cast<const int2 *>(r->d_fixed) + N;
    }
    a.pitch = (size_t)src_pitch;
    a.src_frame = (size_t)src_pitch * src_height;
    a.sw = src_width;
    a.sh = src_height;
    a.W = W;
    a.H = H;
    a.batch = batch;
    a.scale_x = 1.0 / ((double)W / src_width);  // resize.cpp: scale = 1 / inv_scale
    a.scale_y = 1.0 / ((double)H / src_height);
    a.area2 = (src_width == 2 * W && src_height == 2 * H) ? 1 : 0;
    if (!resize) {
        e = sv::launch_rig_pass(remap ? sv::RIG_PASS_GRAY_REMAP : sv::RIG_PASS_GRAY, pixel_format, a, st);
    } else if (!remap) {
        e = sv::launch_rig_pass(sv::RIG_PASS_RESIZE_GRAY, pixel_format, a, st);
    } else {
        // resized gray of both sides in a stream-ordered scratch buffer, then the remap into the outputs
        uint8_t *tmp = nullptr;
        if ((e = hipMallocAsync((void **)&tmp, 2 * N * batch, st)) != hipSuccess) return fail(err, SV_ERR_HIP, std::string("hipMallocAsync: ") + hipGetErrorString(e));
        sv::RigArgs p1 = a;
        p1.dst[0] = tmp;
        p1.dst[1] = tmp + N * batch;
        e = sv::launch_rig_pass(sv::RIG_PASS_RESIZE_GRAY, pixel_format, p1, st);
        if (e == hipSuccess) {
            sv::RigArgs p2 = a;
            p2.src[0] = tmp;
            p2.src[1] = tmp + N * batch;
            p2.colours = nullptr;
            p2.pitch = (size_t)W;
            p2.src_frame = N;
            p2.sw = W;
            p2.sh = H;
            e = sv::launch_rig_pass(sv::RIG_PASS_REMAP, SV_PIX_GRAY8, p2, st);
        }
        const hipError_t ef = hipFreeAsync(tmp, st);
        if (e == hipSuccess) e = ef;
    }
    if (e != hipSuccess) return fail(err, SV_ERR_HIP, std::string("front-end launch: ") + hipGetErrorString(e));
    return SV_OK;
}

} /* extern "C" */
