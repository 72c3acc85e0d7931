// What the stage entries of groups (D) to (AC) of include/stereo_vision_hip.h share on the host (top_view.cpp ... place.cpp): the
// refusal of a bad call, the checks that several groups state in the same words, and the set-up of sv::ReprojectArgs.  Host code only:
// no .hip file includes it.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/stereo_vision_hip.h"
#include "reproject.h"

void sv_internal_set_error(const char *msg);  // engine.cpp: the text sv_last_error(NULL) returns on this thread (it copies msg)

namespace sv {
namespace glue {

constexpr int MAP_CELL_MAX = 1 << 24;  // |top|, |left| of a world map stay below it (sv::OCCMAP_CELL_MAX: occupancy_map.cpp asserts it)

inline int refuse(const char *msg) {
    sv_internal_set_error(msg);
    return SV_ERR_ARG;
}

// "<prefix>: <body>" for the checks below, whose bodies are the same for every entry.  The text lives in a buffer of the calling thread
// until the next call: long enough to hand it to refuse(), or to drop it where only the verdict counts (the *_workspace_bytes entries).
inline const char *prefixed(const char *prefix, const std::string &body) {
    static thread_local std::string text;
    text = std::string(prefix) + ": " + body;
    return text.c_str();
}

// NULL for a batch of frames every kernel can index, else what is wrong with it; max_height 0 = no limit of its own.
inline const char *check_frame(const char *prefix, int batch, int width, int height, int max_height) {
    if (batch < 0 || batch > 65535) return prefixed(prefix, "batch outside 0..65535");
    if (width < 1 || height < 1) return prefixed(prefix, "width or height < 1");
    if (max_height > 0 && height > max_height) return prefixed(prefix, "height > " + std::to_string(max_height));
    if ((int64_t)width * height >= ((int64_t)1 << 31)) return prefixed(prefix, "width * height >= 2^31");
    return nullptr;
}

// NULL for a batch of images that groups (Z) and (AA) can index - at most 8192 x 8192 -, else what is wrong with it.
inline const char *check_images(const char *prefix, int batch, int width, int height) {
    if (const char *bad = check_frame(prefix, batch, width, height, 8192)) return bad;
    if (width > 8192) return prefixed(prefix, "width > 8192");
    return nullptr;
}

// NULL for the camera words the specs of groups (Z), (AA) and (AB) begin with - f, cx, cy, b16, fb, fb16 -, else what is wrong with them.
template <class Spec>
inline const char *check_camera_words(const char *prefix, const Spec *s) {
    const double w[6] = {s->f, s->cx, s->cy, s->b16, s->fb, s->fb16};
    for (double v : w)
        if (!isfinite(v)) return prefixed(prefix, "a word of the camera is not finite");
    if (!(s->f > 0.0) || !(s->b16 > 0.0) || !(s->fb > 0.0) || !(s->fb16 > 0.0)) return prefixed(prefix, "f, b16, fb and fb16 must be > 0");
    return nullptr;
}

// NULL for the rows and columns a world map may have, else what is wrong with them: for the entries that take the two numbers bare.
inline const char *check_map_shape(const char *prefix, int rows, int cols) {
    if (rows < 1 || rows > 32768 || cols < 1 || cols > 32768) return prefixed(prefix, "rows or cols outside 1..32768");
    return nullptr;
}

// NULL for a good map spec, else what is wrong with it: the rules of the fuse entry, which every reader of the map repeats.
inline const char *check_map(const char *prefix, const sv_occupancy_map_spec *m) {
    if (!m) return prefixed(prefix, "the map spec is NULL");
    for (int k = 0; k < 7; k++)
        if (m->reserved[k] != 0) return prefixed(prefix, "a reserved word of the map spec is not 0");
    if (check_map_shape(prefix, m->rows, m->cols)) return prefixed(prefix, "rows or cols of the map outside 1..32768");
    if (m->scale < 1) return prefixed(prefix, "the map's scale < 1");
    if (m->top <= -MAP_CELL_MAX || m->top >= MAP_CELL_MAX || m->left <= -MAP_CELL_MAX || m->left >= MAP_CELL_MAX)
        return prefixed(prefix, "|top| or |left| of the map is 2^24 or more");
    if (m->l_occ < 1 || m->l_occ > 32767 || m->l_free < 1 || m->l_free > 32767) return prefixed(prefix, "l_occ or l_free outside 1..32767");
    if (!(-32767 <= m->l_min && m->l_min <= 0 && 0 <= m->l_max && m->l_max <= 32767) || m->l_min == m->l_max)
        return prefixed(prefix, "the clamp needs -32767 <= l_min <= 0 <= l_max <= 32767 and l_min < l_max");
    return nullptr;
}

inline bool misaligned(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }  // a: a power of two

template <class... P>
inline bool any_misaligned(unsigned a, const P *...p) { return (... || misaligned(p, a)); }  // NULL is aligned

// NULL for a voxel map spec and a buffer that (Q)'s clear entry admits, else what is wrong with them: the check of every entry of (Q)
// to (Y).  nc = the cells per axis, log2_slots = of the table; sv_voxel_map_slots (voxel_map.cpp) holds the rule of the capacity.
inline const char *check_voxel_map(const char *prefix, const void *map, size_t map_bytes, const sv_voxel_map_spec *s, int *nc, int *log2_slots) {
    if (!s) return prefixed(prefix, "spec is NULL");
    for (int k = 0; k < 7; k++)
        if (s->reserved[k] != 0) return prefixed(prefix, "a reserved word of the spec is not 0");
    if (!(s->size > 0.0) || !isfinite(s->size)) return prefixed(prefix, "size is not a finite number > 0");
    for (int k = 0; k < 3; k++) {
        if (!isfinite(s->lo[k]) || !isfinite(s->hi[k])) return prefixed(prefix, "the box must be finite");
        if (!(s->lo[k] < s->hi[k])) return prefixed(prefix, "the box needs lo < hi on every axis");
        const double cells = ceil((s->hi[k] - s->lo[k]) / s->size);  // +inf where the difference or the quotient overflows
        if (!(cells <= 1048576.0)) return prefixed(prefix, "more than 2^20 cells on an axis");
        nc[k] = cells < 1.0 ? 1 : (int)cells;
    }
    const int64_t slots = sv_voxel_map_slots(s->capacity);
    if (slots < 0) return prefixed(prefix, "capacity outside 1 .. 2^26");
    if (!map || misaligned(map, 16) || map_bytes < sv_voxel_map_bytes(s->capacity))
        return prefixed(prefix, "the map is NULL, not 16-byte aligned or smaller than sv_voxel_map_bytes");
    *log2_slots = 0;
    while (((int64_t)1 << *log2_slots) < slots) (*log2_slots)++;
    return nullptr;
}

// Q, and XR / XT or the identity where they are NULL, as launch_reproject_batch (legacy_kernels.hip) sets them up.
inline void set_reproject(ReprojectArgs &rp, const double *Q16, const double *XR9, const double *XT3) {
    for (int i = 0; i < 16; i++) rp.Q[i] = Q16[i];
    rp.has_xf = (XR9 || XT3) ? 1 : 0;
    for (int i = 0; i < 9; i++) rp.XR[i] = XR9 ? XR9[i] : (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; i++) rp.XT[i] = XT3 ? XT3[i] : 0.0;
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// Do the pn bytes at p and the qn bytes at q share a byte?  Never with a NULL pointer.
inline bool overlap(const void *p, size_t pn, const void *q, size_t qn) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && a < b + qn && b < a + pn;
}

// The arguments of a call as spans of bytes, the inputs first: does an output - spans[first_out] and everything behind it - share a
// byte with an input or with an output before it?  A span of no bytes shares none.
struct Span { const void *p; size_t n; };
inline bool outputs_overlap(const Span *spans, int n_spans, int first_out) {
    for (int o = first_out; o < n_spans; o++)
        for (int j = 0; j < o; j++)
            if (spans[o].n && spans[j].n && overlap(spans[o].p, spans[o].n, spans[j].p, spans[j].n)) return true;
    return false;
}

}  // namespace glue
}  // namespace sv
