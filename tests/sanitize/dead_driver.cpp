// Drives the host routine of the dead-key row rule (stringsearchlib_amd/csrc/ngs_set.h: drop_dead_row)
// for tests/test_set_dead_host.py, built with g++ alone (-fsanitize=address,undefined).
//
//   dead_driver IN OUT
// IN is a sequence of records of u32: n, stride, n_keys, limit, mask words (0: no mask, a null pointer),
// then counts[n], keys[n * stride], score bits[n * stride], mask[words].
// -> OUT: counts[n], the number of short rows, then for every row its first counts[i] key ids and its
// first counts[i] score bits.
// Every array is copied into a buffer sized exactly, so an access past a row, the block or the mask is
// a sanitizer report. Prints "ok <records>" and exits 0, or a message and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ngs_set.h"

static int fail(const char* what, size_t i) {
    std::fprintf(stderr, "dead_driver: %s at record %zu\n", what, i);
    return 1;
}

template <class T>
static bool get(std::FILE* in, std::vector<T>& v, size_t n) {
    v.assign(n, T());
    v.shrink_to_fit();
    return !n || std::fread(v.data(), sizeof(T), n, in) == n;
}
template <class T>
static bool put(std::FILE* out, const T* p, size_t n) {
    return !n || std::fwrite(p, sizeof(T), n, out) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: dead_driver IN OUT", 0);
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return fail("cannot open the files", 0);
    size_t rec = 0;
    std::vector<uint32_t> h;
    for (; get(in, h, 5); ++rec) {
        const uint32_t n = h[0], stride = h[1], n_keys = h[2], limit = h[3], words = h[4];
        std::vector<uint32_t> counts, keys, mask;
        std::vector<float> scores;
        if (!get(in, counts, n) || !get(in, keys, (size_t)n * stride) || !get(in, scores, (size_t)n * stride) ||
            !get(in, mask, words))
            return fail("short input", rec);
        if (n_keys && (size_t)words * 32u < n_keys) return fail("the mask is too small", rec);
        uint32_t n_short = 0;
        for (uint32_t i = 0; i < n; ++i) {
            // the row alone in a buffer of its own: a write into a neighbouring row is a report too
            std::vector<uint32_t> k(keys.begin() + (size_t)i * stride, keys.begin() + (size_t)(i + 1) * stride);
            std::vector<float> s(scores.begin() + (size_t)i * stride, scores.begin() + (size_t)(i + 1) * stride);
            k.shrink_to_fit();
            s.shrink_to_fit();
            bool is_short = false;
            counts[i] = ngs::drop_dead_row(counts[i], stride, k.data(), s.data(), words ? mask.data() : nullptr, n_keys,
                                           limit, &is_short);
            if (counts[i] > stride) return fail("a count above the stride", rec);
            n_short += is_short ? 1u : 0u;
            std::copy(k.begin(), k.end(), keys.begin() + (size_t)i * stride);
            std::copy(s.begin(), s.end(), scores.begin() + (size_t)i * stride);
        }
        if (!put(out, counts.data(), n) || !put(out, &n_short, 1)) return fail("cannot write", rec);
        for (uint32_t i = 0; i < n; ++i)
            if (!put(out, keys.data() + (size_t)i * stride, counts[i]) ||
                !put(out, scores.data() + (size_t)i * stride, counts[i]))
                return fail("cannot write", rec);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write", rec);
    std::printf("ok %zu\n", rec);
    return 0;
}
