// Stand-alone host program: the argument checks of group (Z) (csrc/flow.cpp) under AddressSanitizer + UBSan.  The kernels' launchers are
// replaced by stubs that count their calls: a refused call must not reach them, an admitted one must.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "stereo_vision_hip.h"  // -I include
#include "flow_kernels.h"

static int g_launches = 0;
static std::string g_error;
void sv_internal_set_error(const char *msg) { g_error = msg ? msg : ""; }
namespace sv {
hipError_t launch_flow_match(const FlowMatchArgs &, hipStream_t) { g_launches++; return hipSuccess; }
hipError_t launch_flow_sums(const FlowSumsArgs &, hipStream_t) { g_launches++; return hipSuccess; }
}  // namespace sv

static int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { g_bad++; printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); } } while (0)

static sv_flow_spec good_spec() {
    sv_flow_spec s;
    memset(&s, 0, sizeof(s));
    s.f = 40.0, s.cx = 15.5, s.cy = 11.5, s.b16 = 8.0, s.fb = 20.0, s.fb16 = 320.0;
    s.step = 4, s.r = 2, s.wx = 2, s.wy = 2, s.ratio = 230, s.max_cost = 57375, s.capacity = 16;
    return s;
}

int main() {
    alignas(16) static unsigned char buf[1 << 16];  // stands in for device memory: the stubs touch nothing
    void *p = buf;
    size_t need = 77;
    sv_flow_spec s = good_spec();
    // the workspace calls
    EXPECT(sv_flow_match_workspace(32, 24, 1, &s, &need) == SV_OK && need == 8 * 6 * 32);
    EXPECT(sv_flow_match_workspace(32, 24, 1, &s, NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_workspace(32, 24, 1, NULL, &need) == SV_ERR_ARG);
    EXPECT(sv_flow_match_workspace(0, 24, 1, &s, &need) == SV_ERR_ARG && sv_flow_match_workspace(32, 8193, 1, &s, &need) == SV_ERR_ARG);
    EXPECT(sv_flow_match_workspace(8193, 24, 1, &s, &need) == SV_ERR_ARG && sv_flow_match_workspace(32, 24, 65536, &s, &need) == SV_ERR_ARG);
    EXPECT(sv_flow_match_workspace(32, 24, -1, &s, &need) == SV_ERR_ARG && need == 8 * 6 * 32);
    EXPECT(sv_flow_pose_sums_workspace(700, 3, &need) == SV_OK && need == 3 * 3 * 32 * 8);
    EXPECT(sv_flow_pose_sums_workspace(0, 3, &need) == SV_OK && need == 0);
    EXPECT(sv_flow_pose_sums_workspace(65537, 1, &need) == SV_ERR_ARG && sv_flow_pose_sums_workspace(-1, 1, &need) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_workspace(16, 65536, &need) == SV_ERR_ARG && sv_flow_pose_sums_workspace(16, 1, NULL) == SV_ERR_ARG);
    // each bad word of the spec
    struct Word { const char *name; void (*set)(sv_flow_spec &); };
    const Word words[] = {
        {"step 0", [](sv_flow_spec &w) { w.step = 0; }}, {"r 0", [](sv_flow_spec &w) { w.r = 0; }}, {"r 8", [](sv_flow_spec &w) { w.r = 8; }},
        {"wx -1", [](sv_flow_spec &w) { w.wx = -1; }}, {"wy 8193", [](sv_flow_spec &w) { w.wy = 8193; }}, {"candidates", [](sv_flow_spec &w) { w.wx = 64, w.wy = 64; }},
        {"LDS", [](sv_flow_spec &w) { w.r = 4, w.wx = 64, w.wy = 51; }}, {"ratio 257", [](sv_flow_spec &w) { w.ratio = 257; }}, {"ratio -1", [](sv_flow_spec &w) { w.ratio = -1; }},
        {"max_cost -1", [](sv_flow_spec &w) { w.max_cost = -1; }}, {"capacity 65537", [](sv_flow_spec &w) { w.capacity = 65537; }}, {"capacity -1", [](sv_flow_spec &w) { w.capacity = -1; }},
        {"f 0", [](sv_flow_spec &w) { w.f = 0.0; }}, {"cx nan", [](sv_flow_spec &w) { w.cx = __builtin_nan(""); }}, {"cy inf", [](sv_flow_spec &w) { w.cy = __builtin_inf(); }},
        {"b16 -1", [](sv_flow_spec &w) { w.b16 = -1.0; }}, {"fb 0", [](sv_flow_spec &w) { w.fb = 0.0; }}, {"fb16 nan", [](sv_flow_spec &w) { w.fb16 = __builtin_nan(""); }},
        {"reserved", [](sv_flow_spec &w) { w.reserved[8] = 1; }}};
    for (const Word &w : words) {
        sv_flow_spec t = good_spec();
        w.set(t);
        g_error.clear();
        const int rc = sv_flow_match_device(p, p, (const float *)p, NULL, NULL, 1, 32, 24, &t, (int32_t *)p, (int32_t *)p, (int32_t *)p, p, sizeof(buf), NULL);
        if (rc != SV_ERR_ARG || g_error.empty()) g_bad++, printf("FAILED: %s was admitted\n", w.name);
    }
    EXPECT(g_launches == 0);
    // pointers, batch and workspace of the match call
    int32_t *i = (int32_t *)p;
    const float *fl = (const float *)p;
    EXPECT(sv_flow_match_device(NULL, p, fl, NULL, NULL, 1, 32, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, NULL, fl, NULL, NULL, 1, 32, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, NULL, NULL, NULL, 1, 32, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, NULL, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, &s, NULL, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, &s, i, NULL, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, &s, i, i, NULL, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, &s, i, i, i, NULL, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, &s, i, i, i, p, 8 * 6 * 32 - 1, NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, -1, 32, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 65536, 32, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 0, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, (const float *)(buf + 2), NULL, NULL, 1, 32, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, (const float *)(buf + 1), NULL, 1, 32, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, (const double *)(buf + 4), 1, 32, 24, &s, i, i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, &s, (int32_t *)(buf + 2), i, i, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, &s, i, i, i, buf + 2, sizeof(buf) - 2, NULL) == SV_ERR_ARG);
    EXPECT(g_launches == 0);
    EXPECT(sv_flow_match_device(NULL, NULL, NULL, NULL, NULL, 0, 32, 24, &s, NULL, NULL, NULL, NULL, 0, NULL) == SV_OK && g_launches == 0);  // batch 0: nothing to do
    EXPECT(sv_flow_match_device(p, p, fl, fl, (const double *)p, 1, 32, 24, &s, i, i, i, p, 8 * 6 * 32, NULL) == SV_OK && g_launches == 1);
    sv_flow_spec none = good_spec();
    none.capacity = 0;
    EXPECT(sv_flow_match_device(p, p, fl, NULL, NULL, 1, 32, 24, &none, NULL, NULL, i, p, sizeof(buf), NULL) == SV_OK && g_launches == 2);  // no rows: no row pointers
    // the sums call
    int64_t *o = (int64_t *)p;
    const double *d = (const double *)p;
    g_launches = 0;
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, NULL, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, -1, 16, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 65536, 16, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, -1, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 65537, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, -1, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, (1 << 20) + 1, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, 16, -1, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, 16, (1 << 20) + 1, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(NULL, i, d, 1, 16, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, NULL, d, 1, 16, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, NULL, 1, 16, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, 16, 16, NULL, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, 16, 16, o, NULL, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, 16, 16, o, p, 255, NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device((const int32_t *)(buf + 2), i, d, 1, 16, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, (const double *)(buf + 4), 1, 16, &s, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, 16, 16, (int64_t *)(buf + 4), p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, 16, 16, o, buf + 4, sizeof(buf) - 4, NULL) == SV_ERR_ARG);
    sv_flow_spec cam = good_spec();
    cam.fb = __builtin_nan("");
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &cam, 16, 16, o, p, sizeof(buf), NULL) == SV_ERR_ARG);
    EXPECT(g_launches == 0);
    EXPECT(sv_flow_pose_sums_device(NULL, NULL, NULL, 0, 16, &s, 16, 16, NULL, NULL, 0, NULL) == SV_OK && g_launches == 0);
    EXPECT(sv_flow_pose_sums_device(i, i, d, 1, 16, &s, 0, 1 << 20, o, p, 256, NULL) == SV_OK && g_launches == 1);
    EXPECT(sv_flow_pose_sums_device(NULL, i, d, 1, 0, &s, 16, 16, o, NULL, 0, NULL) == SV_OK && g_launches == 2);  // no rows: no matches, no workspace
    printf("launches: %d\nmismatches: %d\n", g_launches, g_bad);
    return g_bad ? 1 : 0;
}
