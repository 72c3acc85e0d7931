// Stand-alone host program: the argument checks of group (AA) (csrc/warp.cpp) under AddressSanitizer + UBSan.  The kernels' launcher is
// replaced by a stub that counts its calls: a refused call must not reach it, an admitted one must.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "stereo_vision_hip.h"  // -I include
#include "warp_kernels.h"

static int g_launches = 0;
static std::string g_error;
void sv_internal_set_error(const char *msg) { g_error = msg ? msg : ""; }
namespace sv {
hipError_t launch_disparity_warp(const WarpArgs &, hipStream_t) { g_launches++; return hipSuccess; }
}  // namespace sv

static int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { g_bad++; printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); } } while (0)

static sv_warp_spec good_spec() {
    sv_warp_spec s;
    memset(&s, 0, sizeof(s));
    s.f = 40.0, s.cx = 15.5, s.cy = 11.5, s.b16 = 8.0, s.fb = 20.0, s.fb16 = 320.0;
    s.e_max = 1, s.tol_q = 16, s.rel_q = 0, s.mode = 0;
    return s;
}

enum { W = 32, H = 24, N = W * H };

int main() {
    alignas(16) static unsigned char buf[16 * N * 4];  // stands in for device memory: the stub touches nothing
    // a 24 x 32 frame: d_prev, d_cur, expected, source, out of 4 N bytes each, label of N bytes, counts, poses, then 8 N bytes of workspace
    const float *dp = (const float *)buf, *dc = (const float *)(buf + 4 * N);
    int32_t *ex = (int32_t *)(buf + 8 * N), *src = (int32_t *)(buf + 12 * N);
    float *out = (float *)(buf + 16 * N);
    uint8_t *lab = buf + 20 * N;
    int32_t *cnt = (int32_t *)(buf + 21 * N);
    const double *pose = (const double *)(buf + 22 * N);
    unsigned char *ws = buf + 24 * N;
    const size_t ws_bytes = 8 * N;
    size_t need = 77;
    sv_warp_spec s = good_spec();
    // the workspace call
    EXPECT(sv_disparity_warp_workspace(W, H, 3, &need) == SV_OK && need == 3 * 8 * N);
    EXPECT(sv_disparity_warp_workspace(W, H, 0, &need) == SV_OK && need == 0);
    need = 77;
    EXPECT(sv_disparity_warp_workspace(W, H, 1, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_workspace(0, H, 1, &need) == SV_ERR_ARG && sv_disparity_warp_workspace(W, 0, 1, &need) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_workspace(8193, H, 1, &need) == SV_ERR_ARG && sv_disparity_warp_workspace(W, 8193, 1, &need) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_workspace(W, H, -1, &need) == SV_ERR_ARG && sv_disparity_warp_workspace(W, H, 65536, &need) == SV_ERR_ARG && need == 77);
    EXPECT(sv_disparity_warp_workspace(8192, 8192, 65535, &need) == SV_OK && need == (size_t)65535 * 8192 * 8192 * 8);  // no overflow
    // each bad word of the spec
    struct Word { const char *name; void (*set)(sv_warp_spec &); };
    const Word words[] = {
        {"e_max -1", [](sv_warp_spec &w) { w.e_max = -1; }}, {"e_max 5", [](sv_warp_spec &w) { w.e_max = 5; }}, {"tol_q -1", [](sv_warp_spec &w) { w.tol_q = -1; }},
        {"tol_q 2^20 + 1", [](sv_warp_spec &w) { w.tol_q = (1 << 20) + 1; }}, {"rel_q -1", [](sv_warp_spec &w) { w.rel_q = -1; }}, {"rel_q 257", [](sv_warp_spec &w) { w.rel_q = 257; }},
        {"mode -1", [](sv_warp_spec &w) { w.mode = -1; }}, {"mode 3", [](sv_warp_spec &w) { w.mode = 3; }},
        {"f 0", [](sv_warp_spec &w) { w.f = 0.0; }}, {"cx nan", [](sv_warp_spec &w) { w.cx = __builtin_nan(""); }}, {"cy inf", [](sv_warp_spec &w) { w.cy = __builtin_inf(); }},
        {"b16 -1", [](sv_warp_spec &w) { w.b16 = -1.0; }}, {"fb 0", [](sv_warp_spec &w) { w.fb = 0.0; }}, {"fb16 nan", [](sv_warp_spec &w) { w.fb16 = __builtin_nan(""); }},
        {"reserved", [](sv_warp_spec &w) { w.reserved[11] = 1; }}};
    for (const Word &w : words) {
        sv_warp_spec t = good_spec();
        w.set(t);
        g_error.clear();
        const int rc = sv_disparity_warp_device(dp, dc, pose, 1, W, H, &t, ex, src, lab, out, cnt, ws, ws_bytes, NULL);
        if (rc != SV_ERR_ARG || g_error.empty()) g_bad++, printf("FAILED: %s was admitted\n", w.name);
    }
    EXPECT(g_launches == 0);
    // pointers, batch, shape and workspace
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, NULL, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(NULL, dc, pose, 1, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, NULL, 1, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, NULL, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, NULL, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, NULL, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, NULL, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, out, NULL, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, out, cnt, NULL, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes - 1, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, -1, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 65536, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, 0, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, 8193, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device((const float *)(buf + 2), dc, pose, 1, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, (const float *)(buf + 4 * N + 1), pose, 1, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, (const double *)(buf + 22 * N + 4), 1, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, (int32_t *)(buf + 8 * N + 2), src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, (int32_t *)(buf + 12 * N + 1), lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, (float *)(buf + 16 * N + 2), cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, out, (int32_t *)(buf + 21 * N + 2), ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, out, cnt, ws + 4, ws_bytes, NULL) == SV_ERR_ARG);
    // an output on an input, on another output, on the workspace
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, (float *)dc, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, (int32_t *)dp, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, ex, lab, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, (uint8_t *)out + 5, out, cnt, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, out, (int32_t *)pose, ws, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, out, cnt, (void *)src, ws_bytes, NULL) == SV_ERR_ARG);
    EXPECT(g_launches == 0);
    EXPECT(sv_disparity_warp_device(NULL, NULL, NULL, 0, W, H, &s, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL) == SV_OK && g_launches == 0);  // batch 0: nothing to do
    EXPECT(sv_disparity_warp_device(dp, dc, pose, 1, W, H, &s, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_OK && g_launches == 1);
    EXPECT(sv_disparity_warp_device(dp, NULL, pose, 1, W, H, &s, ex, src, NULL, NULL, cnt, ws, ws_bytes, NULL) == SV_OK && g_launches == 2);  // no d_cur: no label, no out
    sv_warp_spec all = good_spec();
    all.e_max = 4, all.tol_q = 1 << 20, all.rel_q = 256, all.mode = 2;
    EXPECT(sv_disparity_warp_device(dp, dp, pose, 1, W, H, &all, ex, src, lab, out, cnt, ws, ws_bytes, NULL) == SV_OK && g_launches == 3);  // the inputs may share bytes
    printf("launches: %d\nmismatches: %d\n", g_launches, g_bad);
    return g_bad ? 1 : 0;
}
