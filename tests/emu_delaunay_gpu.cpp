// CPU emulation of csrc/delaunay_gpu.hip: the device functions compiled as plain C++, the tree processed depth by depth with
// the nodes of one depth in arbitrary (here: reversed) order, against Delaunay::triangulate.  tests/test_sanitizers.py builds it
// with AddressSanitizer.  Every loop trip of every merge counts against a bound derived from the size of the node being merged
// (delaunay_gpu.hip: DgEmu, emulation only): a seam walk that would not terminate on the GPU ends here and fails with the set's name.
// argv[1]: the structured sets of tests/degenerate_sets.py (tests/corpus_file.h).
#define DG_HOST_EMULATION 1
#define __device__
#define __host__
#define __forceinline__ inline
#include "delaunay_gpu.hip"
#include "host_stage.h"
#include "corpus_file.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static int bad = 0;

// 1: every coordinate difference is below 2^14 (what the launchers pass as `narrow`: the 32-bit in-circle terms are exact)
static bool is_narrow(const int32_t *xy, int n) {
    int32_t lo[2] = {xy[0], xy[1]}, hi[2] = {xy[0], xy[1]};
    for (int i = 0; i < n; i++)
        for (int c = 0; c < 2; c++) lo[c] = std::min(lo[c], xy[2 * i + c]), hi[c] = std::max(hi[c], xy[2 * i + c]);
    return (int64_t)hi[0] - lo[0] < (1 << 14) && (int64_t)hi[1] - lo[1] < (1 << 14);
}

static void report(const char *what, const char *name, int n, int m, int nw, size_t got) {
    bad++;
    if (bad < 12) printf("%s: set %s n %d m %d  tris %d vs %zu\n", what, name, n, m, nw, got);
}

static bool budget_ok(const char *name, int n, int m) {
    const uint32_t over = sv::dg::dg_emu.overruns;
    sv::dg::dg_emu.overruns = 0;
    if (over) {
        bad++;
        printf("trip-count bound exceeded in %u merges: set %s n %d m %d\n", over, name, n, m);
    }
    return over == 0;
}

// A set that fits LDS whole (k_delaunay / dg_build_and_emit).  Returns false when the set is not one for this path.
template <bool NARROW>
static bool run_whole(const int32_t *xy, int n, const char *name) {
    sv::Delaunay dl;
    std::vector<int32_t> want(6 * (size_t)n + 24), ids(n);
    const int nw = dl.triangulate(xy, n, want.data(), 2 * n + 8);
    sv::Delaunay dl2;
    const int m = dl2.kd_ordered_ids(xy, n, ids.data());
    if (m < 3) {
        if (nw != 0) report("mismatch", name, n, m, nw, 0);
        return true;
    }
    if (n > 0xFFFE || m > sv::dg::DG_SUB_MAX) return false;  // (16-bit vertex ids; the LDS limit)
    const int nslots = 2 * m - 1;
    const int depth = sv::dg::dg_depth(m);
    std::vector<uint32_t> res(2 << depth, 0);
    std::vector<sv::dg::DTri> T(nslots);
    std::vector<uint32_t> pxy(n);
    std::vector<uint16_t> ord(m);
    for (int i = 0; i < n; i++) pxy[i] = ((uint32_t)xy[2 * i] & 0xFFFFu) | ((uint32_t)xy[2 * i + 1] << 16);
    for (int i = 0; i < m; i++) ord[i] = (uint16_t)ids[i];
    T[0].w[0] = 0, T[0].w[1] = 0xFFFFu << 16, T[0].w[2] = 0xFFFFFFFFu;
    const sv::dg::Mesh M{&T[0].w[0], pxy.data()};
    const uint16_t *F = reinterpret_cast<const uint16_t *>(T.data());
    for (int d = depth; d >= 0; d--)
        for (int j = (1 << d) - 1; j >= 0; j--) sv::dg::d_process_node<NARROW>(M, res.data(), ord.data(), m, d, j);
    if (!budget_ok(name, n, m)) return true;
    std::vector<int32_t> got;
    for (int t = 1; t < nslots; t++) {
        if (F[6 * t + 3] == 0xFFFF || F[6 * t + 4] == 0xFFFF || F[6 * t + 5] == 0xFFFF) continue;
        got.push_back(F[6 * t + 4]); got.push_back(F[6 * t + 5]); got.push_back(F[6 * t + 3]);
    }
    if ((int)got.size() != 3 * nw || (!got.empty() && memcmp(got.data(), want.data(), sizeof(int32_t) * got.size()))) report("mismatch", name, n, m, nw, got.size() / 3);
    return true;
}

// A set cut into subtrees (dg_subtree / dg_top of the kernels, restated sequentially): every subtree in a local 16-bit mesh with local
// vertex numbers, exported into one 32-bit mesh, then the merges above the cut.  Returns the cut depth, or -1 when the set is not one
// for this path (it fits a subtree whole, or needs more subtrees than a set may have).
template <bool NARROW>
static int run_cut(const int32_t *xy, int n, int sub_max, const char *name) {
    sv::Delaunay dl;
    std::vector<int32_t> want(6 * (size_t)n + 24), ids(n);
    const int nw = dl.triangulate(xy, n, want.data(), 2 * n + 8);
    sv::Delaunay dl2;
    const int m = dl2.kd_ordered_ids(xy, n, ids.data());
    if (m <= sub_max) return -1;  // (many duplicates: the set fits LDS after all - run_whole's case)
    const int c = sv::dg::dg_cut_depth(m, sub_max);
    if (c > sv::dg::DG_CUT_MAX) return -1;
    std::vector<sv::dg::GTri> G(2 * (size_t)m);
    std::vector<uint32_t> gres(4 << sv::dg::DG_CUT_MAX, 0);
    for (int k = 0; k < 3; k++) { G[0].w[k] = 0; G[0].w[3 + k] = sv::dg::GHOST32; }
    for (int j = (1 << c) - 1; j >= 0; j--) {
        int lo, ns, axis0;
        uint32_t slot0;
        if (!sv::dg::d_node(m, c, j, lo, ns, slot0, axis0)) { bad++; continue; }
        const int depth = sv::dg::dg_depth(ns);
        std::vector<uint32_t> res(2 << depth, 0);
        std::vector<sv::dg::DTri> T(2 * ns - 1);
        std::vector<uint32_t> pxy(ns);
        std::vector<uint16_t> ord(ns);
        for (int i = 0; i < ns; i++) { pxy[i] = ((uint32_t)xy[2 * ids[lo + i]] & 0xFFFFu) | ((uint32_t)xy[2 * ids[lo + i] + 1] << 16); ord[i] = (uint16_t)i; }
        T[0].w[0] = 0, T[0].w[1] = 0xFFFFu << 16, T[0].w[2] = 0xFFFFFFFFu;
        const sv::dg::Mesh M{&T[0].w[0], pxy.data()};
        const uint16_t *F = reinterpret_cast<const uint16_t *>(T.data());
        for (int d = depth; d >= 0; d--)
            for (int q = (1 << d) - 1; q >= 0; q--) sv::dg::d_process_node<NARROW>(M, res.data(), ord.data(), ns, d, q, axis0);
        for (int t = 1; t < 2 * ns - 1; t++)
            for (int k = 0; k < 3; k++) {
                G[slot0 + t - 1].w[k] = sv::dg::dg_global_handle(F[6 * t + k], slot0);
                G[slot0 + t - 1].w[3 + k] = F[6 * t + 3 + k] == 0xFFFF ? sv::dg::GHOST32 : (uint32_t)ids[lo + F[6 * t + 3 + k]];
            }
        gres[2 * ((1 << c) + j)] = sv::dg::dg_global_handle(res[1] & 0xFFFFu, slot0);
        gres[2 * ((1 << c) + j) + 1] = sv::dg::dg_global_handle(res[1] >> 16, slot0);
    }
    const sv::dg::MeshG MG{G.data(), xy, 16u * (uint32_t)m + 4096u};
    for (int d = c - 1; d >= 0; d--)
        for (int j = (1 << d) - 1; j >= 0; j--) sv::dg::dg_top_node<NARROW>(MG, gres.data(), m, d, j);
    if (!budget_ok(name, n, m)) return c;
    std::vector<int32_t> got;
    for (int t = 1; t < 2 * m - 1; t++) {
        if (G[t].w[3] == sv::dg::GHOST32 || G[t].w[4] == sv::dg::GHOST32 || G[t].w[5] == sv::dg::GHOST32) continue;
        got.push_back((int32_t)G[t].w[4]); got.push_back((int32_t)G[t].w[5]); got.push_back((int32_t)G[t].w[3]);
    }
    if ((int)got.size() != 3 * nw || (!got.empty() && memcmp(got.data(), want.data(), sizeof(int32_t) * got.size()))) report("mismatch (cut)", name, n, m, nw, got.size() / 3);
    return c;
}

int main(int argc, char **argv) {
    std::mt19937 rng(11);
    char label[64];
    for (int it = 0; it < 400; it++) {
        int n = 3 + rng() % (it % 10 == 0 ? 3900 : 400);
        std::vector<int32_t> xy(2 * n);
        for (int i = 0; i < n; i++) {
            if (it % 3 == 0) { xy[2 * i] = (int)(rng() % 250) * 5; xy[2 * i + 1] = (int)(rng() % 75) * 5; }
            else if (it % 3 == 1) { xy[2 * i] = (int)(rng() % 1300) - 50; xy[2 * i + 1] = (int)(rng() % 75) * 5; }
            else { xy[2 * i] = (int)(rng() % 12) * 5; xy[2 * i + 1] = (int)(rng() % 12) * 5; }
        }
        snprintf(label, sizeof(label), "random %d", it);
        if (it % 2)  // the engine's sets are narrow (32-bit in-circle terms); both forms must give the same mesh on them
            run_whole<true>(xy.data(), n, label);
        else
            run_whole<false>(xy.data(), n, label);
    }
    // Random sets cut into subtrees; subtree sizes from 7 to 4000.
    int cut_cases = 0, deepest = 0;
    for (int it = 0; it < 120; it++) {
        const int sub_max = it % 4 == 0 ? 4000 : 7 + (int)(rng() % 600);
        int n = sub_max + 1 + (int)(rng() % (it % 4 == 0 ? 30000 : 20 * sub_max));
        if (sv::dg::dg_cut_depth(n, sub_max) > sv::dg::DG_CUT_MAX) n = sub_max << sv::dg::DG_CUT_MAX;
        std::vector<int32_t> xy(2 * n);
        for (int i = 0; i < n; i++) {
            if (it % 3 == 0) { xy[2 * i] = (int)(rng() % 768) * 5; xy[2 * i + 1] = (int)(rng() % 432) * 5; }
            else if (it % 3 == 1) { xy[2 * i] = (int)(rng() % 4000) - 190; xy[2 * i + 1] = (int)(rng() % 432) * 5; }
            else { xy[2 * i] = (int)(rng() % 60) * 5; xy[2 * i + 1] = (int)(rng() % 60) * 5; }
        }
        snprintf(label, sizeof(label), "random cut %d (sub_max %d)", it, sub_max);
        const int c = run_cut<true>(xy.data(), n, sub_max, label);
        if (c < 0) continue;
        cut_cases++;
        deepest = c > deepest ? c : deepest;
    }
    printf("cut sets: %d, deepest cut %d\n", cut_cases, deepest);
    if (cut_cases < 60 || deepest < 5) bad++;
    // The structured sets: each one whole in LDS where it fits (with the 32-bit in-circle terms where the launchers would choose them,
    // and always with the 64-bit ones), and cut with subtree limits of 6, 50, 333 and 4000 vertices wherever that gives 1 .. 2^6 subtrees.
    if (argc > 1) {
        std::vector<CorpusSet> corpus;
        if (!load_corpus(argv[1], corpus)) {
            printf("cannot read the corpus %s\n", argv[1]);
            return 2;
        }
        int whole = 0, cut = 0, untouched = 0, depths[sv::dg::DG_CUT_MAX + 1] = {0};
        for (const CorpusSet &s : corpus) {
            const int n = s.n();
            const bool narrow = is_narrow(s.xy.data(), n);
            bool ran = false;
            if (n <= 0xFFFE) {
                if (run_whole<false>(s.xy.data(), n, s.name.c_str())) ran = true, whole++;
                // (the launchers choose the 32-bit in-circle terms for narrow sets only: those run a second time with them - any mismatch
                // counts, the run does not - and the cut path below runs with the terms the launcher would choose)
                if (narrow) run_whole<true>(s.xy.data(), n, s.name.c_str());
            }
            for (int sub_max : {6, 50, 333, 4000}) {
                const int c = narrow ? run_cut<true>(s.xy.data(), n, sub_max, s.name.c_str()) : run_cut<false>(s.xy.data(), n, sub_max, s.name.c_str());
                if (c < 0) continue;
                ran = true, cut++, depths[c]++;
            }
            if (!ran) {
                untouched++;
                printf("corpus set %s (%d points) fits neither path\n", s.name.c_str(), n);
            }
        }
        printf("corpus sets: %d (whole in LDS: %d, cut runs: %d, by cut depth 1..6: %d %d %d %d %d %d, beyond both paths: %d)\n", (int)corpus.size(), whole, cut, depths[1],
               depths[2], depths[3], depths[4], depths[5], depths[6], untouched);
        for (int c = 1; c <= sv::dg::DG_CUT_MAX; c++)
            if (!depths[c]) bad++;
    }
    printf("largest share of its trip-count bound a merge used: %u / 1000\n", sv::dg::dg_emu.worst_permille);
    printf("gpu-delaunay emulation done, mismatches: %d\n", bad);
    return bad != 0;
}
