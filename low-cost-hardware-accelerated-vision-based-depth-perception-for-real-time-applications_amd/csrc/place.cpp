// Group (AC) of include/stereo_vision_hip.h: polar height descriptors of frames of rows, and the search of queries among keys under every
// roll (place_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a
// refused call leaves its text for sv_last_error(NULL).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "place_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

constexpr int PLACE_CAPACITY_MAX = 1 << 24;  // rows per frame: a row's index and a frame's counts stay in 32 bits

std::atomic<int> g_flags{0};  // sv_debug_place

const char *check_shape(const char *prefix, int rings, int sectors) {
    if (rings < 1 || rings > sv::PLACE_RINGS_MAX) return prefixed(prefix, "rings outside 1..64");
    if (sectors < sv::PLACE_SECTORS_MIN || sectors > sv::PLACE_SECTORS_MAX || sectors % 4) return prefixed(prefix, "sectors is no multiple of 4 in 8..128");
    if (rings * sectors > sv::PLACE_BINS_MAX) return prefixed(prefix, "rings * sectors > 4096");
    return nullptr;
}

// NULL for a spec the kernels can use, else what is wrong with it.
const char *check_spec(const char *prefix, const sv_place_spec *s) {
    if (!s) return prefixed(prefix, "spec is NULL");
    for (int k = 0; k < 10; k++)
        if (s->reserved[k] != 0) return prefixed(prefix, "a reserved word of the spec is not 0");
    if (const char *bad = check_shape(prefix, s->rings, s->sectors)) return bad;
    if (!isfinite(s->r_max) || !isfinite(s->z_lo) || !isfinite(s->z_hi) || !isfinite(s->r_min)) return prefixed(prefix, "a word of the spec is not finite");
    if (!(s->r_max > 0.0) || !(s->z_lo < s->z_hi) || !(0.0 <= s->r_min && s->r_min < s->r_max)) return prefixed(prefix, "the spec needs r_max > 0, z_lo < z_hi and 0 <= r_min < r_max");
    const double unit = s->r_max / 1024.0, z_unit = (s->z_hi - s->z_lo) / 255.0;
    if (!(unit > 0.0) || !isfinite(z_unit) || !(z_unit > 0.0)) return prefixed(prefix, "r_max / 1024 or (z_hi - z_lo) / 255 is not a finite number > 0");
    return nullptr;
}

}  // namespace

extern "C" {

int sv_place_descriptor_workspace(int batch, int rings, int sectors, size_t *bytes) {
    if (!bytes) return refuse("sv_place_descriptor_workspace: bytes is NULL");
    if (batch < 0 || batch > sv::PLACE_BATCH_MAX) return refuse("sv_place_descriptor_workspace: batch outside 0..65535");
    if (const char *bad = check_shape("sv_place_descriptor_workspace", rings, sectors)) return refuse(bad);
    *bytes = (size_t)batch * (size_t)(sv::PLACE_HEAD + rings * sectors) * sizeof(uint32_t);
    return SV_OK;
}

int sv_place_descriptor_device(const void *xyz, int dtype, const int32_t *n, const int32_t *counts, const double *poses, int batch, int capacity,
                               const int32_t *dirs, const sv_place_spec *spec, uint8_t *desc, uint8_t *ring, int32_t *words, void *workspace,
                               size_t workspace_bytes, void *stream) {
    if (batch < 0 || batch > sv::PLACE_BATCH_MAX) return refuse("sv_place_descriptor: batch outside 0..65535");
    if (capacity < 0 || capacity > PLACE_CAPACITY_MAX) return refuse("sv_place_descriptor: capacity outside 0..2^24");
    if (dtype != SV_CLOUD_F32 && dtype != SV_CLOUD_F64) return refuse("sv_place_descriptor: dtype is not SV_CLOUD_F32 / SV_CLOUD_F64");
    if (const char *bad = check_spec("sv_place_descriptor", spec)) return refuse(bad);
    if (batch > 0 && (!counts || !dirs || !desc || !ring || !words || !workspace)) return refuse("sv_place_descriptor: counts, dirs, desc, ring, words or the workspace is NULL");
    if (batch > 0 && capacity > 0 && !xyz) return refuse("sv_place_descriptor: xyz is NULL");
    if (misaligned(xyz, dtype == SV_CLOUD_F32 ? 4 : 8)) return refuse("sv_place_descriptor: xyz is not aligned to its element");
    if (misaligned(poses, 8)) return refuse("sv_place_descriptor: poses is not 8-byte aligned");
    if (any_misaligned(4, n, counts, dirs, desc, words) || misaligned(workspace, 4)) return refuse("sv_place_descriptor: n, counts, dirs, desc, words or the workspace is not 4-byte aligned");
    size_t need;
    sv_place_descriptor_workspace(batch, spec->rings, spec->sectors, &need);
    if (workspace_bytes < need) return refuse("sv_place_descriptor: the workspace is smaller than sv_place_descriptor_workspace asks for");
    const size_t B = (size_t)batch, rows = B * (size_t)capacity, bins = (size_t)spec->rings * spec->sectors;
    const Span spans[] = {{xyz, rows * 3 * (dtype == SV_CLOUD_F32 ? 4 : 8)}, {n, rows * 4}, {counts, B * 4}, {poses, B * 96}, {dirs, (size_t)spec->sectors * 8},
                          {workspace, need}, {desc, B * bins}, {ring, B * spec->rings}, {words, B * 16}};
    if (outputs_overlap(spans, 9, 5)) return refuse("sv_place_descriptor: an output or the workspace shares bytes with an input or another output");
    if (batch == 0) return SV_OK;  // nothing to write

    sv::PlaceDescArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = xyz, a.n = n, a.counts = counts, a.poses = poses, a.dirs = dirs;
    a.B = batch, a.cap = capacity, a.f64 = dtype == SV_CLOUD_F64 ? 1 : 0, a.R = spec->rings, a.S = spec->sectors;
    a.n_chunks = (capacity + sv::PLACE_CHUNK - 1) / sv::PLACE_CHUNK;
    a.r_max = spec->r_max, a.z_lo = spec->z_lo, a.z_hi = spec->z_hi;
    a.unit = spec->r_max / 1024.0, a.z_unit = (spec->z_hi - spec->z_lo) / 255.0;
    const double m = floor(spec->r_min / a.unit);  // below 1024: r_min < r_max
    a.r_min2 = (long long)m * (long long)m;
    for (int r = 0; r <= a.R; r++) {
        const int e = sv::PLACE_Q * r / a.R;
        a.edge2[r] = e * e;
    }
    a.work = static_cast<uint32_t *>(workspace), a.desc = desc, a.ring = ring, a.words = words;
    if (sv::launch_place_descriptor(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_place_descriptor: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_place_match_workspace(int queries, int keys, size_t *bytes) {
    if (!bytes) return refuse("sv_place_match_workspace: bytes is NULL");
    if (queries < 0 || queries > sv::PLACE_QUERIES_MAX) return refuse("sv_place_match_workspace: queries outside 0..65535");
    if (keys < 0 || keys > sv::PLACE_KEYS_MAX) return refuse("sv_place_match_workspace: keys outside 0..2^20");
    const size_t groups = ((size_t)keys + sv::PLACE_SHARE - 1) / sv::PLACE_SHARE;
    *bytes = (size_t)queries * groups * sv::PLACE_PART_WORDS * sizeof(int32_t);
    return SV_OK;
}

int sv_place_match_device(const uint8_t *q_desc, const int32_t *q_words, const uint8_t *q_ring, const int32_t *q_seq, int queries, const uint8_t *k_desc,
                          const int32_t *k_words, const uint8_t *k_ring, const int32_t *k_seq, int keys, int rings, int sectors, int min_gap, int ring_gate,
                          int max_shift, int accept, int32_t *best, int32_t *counts, int32_t *pair, void *workspace, size_t workspace_bytes, void *stream) {
    size_t need;
    if (sv_place_match_workspace(queries, keys, &need) != SV_OK) return refuse("sv_place_match: queries outside 0..65535 or keys outside 0..2^20");
    if (const char *bad = check_shape("sv_place_match", rings, sectors)) return refuse(bad);
    if (min_gap < 0) return refuse("sv_place_match: min_gap < 0");
    if (ring_gate < -1) return refuse("sv_place_match: ring_gate < -1");
    if (max_shift < -1 || max_shift > sv::PLACE_SECTORS_MAX) return refuse("sv_place_match: max_shift outside -1..128");
    if (accept < 0 || accept > sv::PLACE_ACCEPT_MAX) return refuse("sv_place_match: accept outside 0..2^20");
    if (queries > 0 && (!q_desc || !q_words || !q_ring || !q_seq || !best || !counts)) return refuse("sv_place_match: q_desc, q_words, q_ring, q_seq, best or counts is NULL");
    if (queries > 0 && keys > 0 && (!k_desc || !k_words || !k_ring || !k_seq || !workspace)) return refuse("sv_place_match: k_desc, k_words, k_ring, k_seq or the workspace is NULL");
    if (any_misaligned(4, q_desc, q_words, q_seq, k_desc, k_words, k_seq) || any_misaligned(4, best, counts, pair) || misaligned(workspace, 4))
        return refuse("sv_place_match: a descriptor, words, sequence numbers, an output or the workspace is not 4-byte aligned");
    if (workspace_bytes < need) return refuse("sv_place_match: the workspace is smaller than sv_place_match_workspace asks for");
    const size_t Q = (size_t)queries, K = (size_t)keys, bins = (size_t)rings * sectors;
    const Span spans[] = {{q_desc, Q * bins}, {q_words, Q * 16}, {q_ring, Q * rings}, {q_seq, Q * 4}, {k_desc, K * bins}, {k_words, K * 16}, {k_ring, K * rings},
                          {k_seq, K * 4}, {workspace, need}, {best, Q * 16}, {counts, Q * 12}, {pair, Q * K * 8}};
    if (outputs_overlap(spans, 12, 8)) return refuse("sv_place_match: an output or the workspace shares bytes with an input or another output");
    if (queries == 0) return SV_OK;  // nothing to write

    sv::PlaceMatchArgs a;
    memset(&a, 0, sizeof(a));
    a.q_desc = q_desc, a.k_desc = k_desc, a.q_words = q_words, a.k_words = k_words, a.q_ring = q_ring, a.k_ring = k_ring, a.q_seq = q_seq, a.k_seq = k_seq;
    a.Q = queries, a.K = keys, a.R = rings, a.S = sectors;
    a.n_groups = (keys + sv::PLACE_SHARE - 1) / sv::PLACE_SHARE;
    a.min_gap = min_gap, a.ring_gate = ring_gate, a.max_shift = max_shift < 0 ? sectors : max_shift, a.accept = accept, a.flags = g_flags.load();
    a.part = static_cast<int32_t *>(workspace), a.best = best, a.counts = counts, a.pair = pair;
    if (sv::launch_place_match(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_place_match: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_place(int flags) {
    if (flags & ~(int)sv::PLACE_FLAGS_MASK) return refuse("sv_debug_place: flags outside 0..1");
    g_flags.store(flags);
    return SV_OK;
}

} /* extern "C" */
