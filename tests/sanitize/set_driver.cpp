// Drives the host routine of the index sets' merge (stringsearchlib_amd/csrc/ngs_set.h) for
// tests/test_set_host.py, built with g++ alone (-fsanitize=address,undefined).
//
//   set_driver IN OUT
// IN is a sequence of records of u32: P, n, limit, out_stride, then for each of the P parts stride, base,
// n_keys, counts[n], keys[n * stride], score bits[n * stride], lens[n_keys].
// -> OUT: counts[n], then for every row its first counts[i] key ids and its first counts[i] score bits.
// Every array is copied into a buffer sized exactly, so an access past a row, a block or a length table
// is a sanitizer report. Prints "ok <records>" and exits 0, or a message and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ngs_set.h"

static int fail(const char* what, size_t i) {
    std::fprintf(stderr, "set_driver: %s at record %zu\n", what, i);
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
    if (argc != 3) return fail("usage: set_driver IN OUT", 0);
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return fail("cannot open the files", 0);
    size_t rec = 0;
    std::vector<uint32_t> h;
    for (; get(in, h, 4); ++rec) {
        const uint32_t P = h[0], n = h[1], limit = h[2], out_stride = h[3];
        if (P == 0 || P > ngs::kSetMaxParts) return fail("bad part count", rec);
        struct Block {
            std::vector<uint32_t> counts, keys, lens;
            std::vector<float> scores;
        };
        std::vector<Block> blocks(P);
        std::vector<ngs::MergePart> parts(P);
        for (uint32_t p = 0; p < P; ++p) {
            std::vector<uint32_t> ph;
            Block& b = blocks[p];
            if (!get(in, ph, 3) || !get(in, b.counts, n) || !get(in, b.keys, (size_t)n * ph[0]) ||
                !get(in, b.scores, (size_t)n * ph[0]) || !get(in, b.lens, ph[2]))
                return fail("short input", rec);
            parts[p] = ngs::MergePart{b.counts.data(), b.keys.data(), b.scores.data(), b.lens.data(), ph[0], ph[1], ph[2], 0u};
        }
        if (out_stride < ngs::merge_min_stride(parts.data(), P, limit)) return fail("the stride is too small", rec);
        std::vector<uint32_t> counts(n), keys((size_t)n * out_stride);
        std::vector<float> scores((size_t)n * out_stride);
        counts.shrink_to_fit();
        keys.shrink_to_fit();
        scores.shrink_to_fit();
        ngs::merge_rows(parts.data(), P, n, limit, out_stride, counts.data(), keys.data(), scores.data());
        if (!put(out, counts.data(), n)) return fail("cannot write", rec);
        for (uint32_t i = 0; i < n; ++i) {
            if (counts[i] > out_stride) return fail("a count above the stride", rec);
            if (!put(out, keys.data() + (size_t)i * out_stride, counts[i]) ||
                !put(out, scores.data() + (size_t)i * out_stride, counts[i]))
                return fail("cannot write", rec);
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write", rec);
    std::printf("ok %zu\n", rec);
    return 0;
}
