// Launch interface of place_kernels.hip (place recognition: polar height descriptors of frames of rows, and the search of query
// descriptors among stored ones under every rotation: place.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

enum {
    PLACE_RINGS_MAX = 64,
    PLACE_SECTORS_MIN = 8,
    PLACE_SECTORS_MAX = 128,
    PLACE_BINS_MAX = 4096,      // rings * sectors: 255 * 4096 < 2^20, so (sad << 8) | shift fits 32 bits
    PLACE_Q = 1024,             // a row's x and y in units of r_max / 1024
    PLACE_THREADS = 256,        // a workgroup of the descriptor's kernels
    PLACE_CHUNK = 4096,         // rows of a frame that one workgroup of the binning kernel takes: 16 per thread
    PLACE_HEAD = 4,             // words in front of a frame's bins in the workspace: kept, dropped, 0, 0
    PLACE_MATCH_THREADS = 256,  // a workgroup of the match kernel: four wavefronts
    PLACE_SHARE = 64,           // keys of a workgroup of the match kernel: a lane each in the tests, sixteen per wavefront in the search
    PLACE_PART_WORDS = 8,       // a workgroup's partial: key, shift, sad, norm, before the gate, behind it, 0, 0
    PLACE_QUERIES_MAX = 65535,
    PLACE_KEYS_MAX = 1 << 20,
    PLACE_BATCH_MAX = 65535,
    PLACE_ACCEPT_MAX = 1 << 20,
    PLACE_ONE_KEY = 1,          // flags bit 0: the search takes one key per pass instead of four (sv_debug_place)
    PLACE_FLAGS_MASK = 1
};

struct PlaceDescArgs {
    const void *xyz;         // [B][cap][3] f32 or f64
    const int32_t *n;        // [B][cap] or NULL
    const int32_t *counts;   // [B]
    const double *poses;     // [B][12] or NULL
    const int32_t *dirs;     // [S][2]
    int B, cap, f64, R, S;
    int n_chunks;            // ceil(cap / PLACE_CHUNK)
    double r_max, z_lo, z_hi, unit, z_unit;
    long long r_min2;
    int edge2[PLACE_RINGS_MAX + 1];
    uint32_t *work;          // workspace: [B][PLACE_HEAD + R * S]
    uint8_t *desc;           // [B][R][S]
    uint8_t *ring;           // [B][R]
    int32_t *words;          // [B][4]
};

struct PlaceMatchArgs {
    const uint8_t *q_desc, *k_desc;    // [Q][R][S], [K][R][S]
    const int32_t *q_words, *k_words;  // [.][4]
    const uint8_t *q_ring, *k_ring;    // [.][R]
    const int32_t *q_seq, *k_seq;      // [.]
    int Q, K, R, S;
    int n_groups;                      // ceil(K / PLACE_SHARE)
    int min_gap, ring_gate, max_shift, accept, flags;
    int32_t *part;                     // workspace: [Q][n_groups][PLACE_PART_WORDS]
    int32_t *best;                     // [Q][4]
    int32_t *counts;                   // [Q][3]
    int32_t *pair;                     // [Q][K][2] or NULL
};

// Three kernels: the workspace cleared; grid (n_chunks, B) - a lane per row, the maxima of a chunk in LDS, flushed by integer atomicMax
// (left out for cap == 0); a workgroup per frame: bytes, ring counts, words.  B >= 1.
hipError_t launch_place_descriptor(const PlaceDescArgs &a, hipStream_t st);

// Two kernels: grid (n_groups, Q) - the tests a lane per key, the search a wavefront per key with a lane per shift, a partial per
// workgroup (left out for K == 0); a workgroup per query: the best of the partials.  Q >= 1.
hipError_t launch_place_match(const PlaceMatchArgs &a, hipStream_t st);

}  // namespace sv
