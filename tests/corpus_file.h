// The structured vertex sets of tests/degenerate_sets.py as the sanitizer / emulation programs read them: tests/test_sanitizers.py writes
// the corpus to a file (int32 count; per set: int32 name length, the name, int32 n, n (x, y) pairs of int32) and passes its path.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <string>
#include <vector>

struct CorpusSet {
    std::string name;
    std::vector<int32_t> xy;
    int n() const { return (int)xy.size() / 2; }
    bool on_lattice(int step) const {  // a support lattice's vertices: rows at multiples of the step
        for (int i = 0; i < n(); i++)
            if (xy[2 * i + 1] % step != 0 || xy[2 * i + 1] < 0) return false;
        return true;
    }
};

// false: the file is missing or cut short (the caller fails: an unreadable corpus must not pass as an empty one)
static bool load_corpus(const char *path, std::vector<CorpusSet> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int32_t count = 0;
    bool ok = fread(&count, 4, 1, f) == 1 && count > 0;
    for (int s = 0; ok && s < count; s++) {
        int32_t len = 0, n = 0;
        CorpusSet c;
        ok = fread(&len, 4, 1, f) == 1 && len > 0 && len < 256;
        if (ok) c.name.resize(len), ok = fread(&c.name[0], 1, len, f) == (size_t)len;
        ok = ok && fread(&n, 4, 1, f) == 1 && n >= 3 && n < (1 << 22);
        if (ok) c.xy.resize(2 * (size_t)n), ok = fread(c.xy.data(), 4, 2 * (size_t)n, f) == 2 * (size_t)n;
        if (ok) out.push_back(std::move(c));
    }
    fclose(f);
    return ok && (int)out.size() == count;
}
