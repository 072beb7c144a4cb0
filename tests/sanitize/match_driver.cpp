// Drives the host routines of the matching stage (stringsearchlib_amd/csrc/ngs_match.h) for
// tests/test_link_host.py, built with g++ alone (-fsanitize=address,undefined).
//
//   match_driver IN OUT
// IN is a sequence of records, each a u32 tag and its fields (u32 unless said otherwise):
//   1 greedy  n_a, n_b, n, stride, first, then counts[n], keys[n * stride], f32 values[n * stride]
//             -> OUT: match_a[n_a], match_b[n_b], the pairs
//   2 rounds  n_a, n_b, n, stride, first, cuts, then row boundaries cut[cuts + 1] (0 .. n, ascending),
//             counts[n], keys[n * stride], f32 values[n * stride]: rounds over the blocks
//             [cut[j], cut[j + 1]) with the flags a caller of several blocks passes (BEGIN | BID on the
//             first, BID on the others, then ACCEPT on each), until a round adds nothing
//             -> OUT: match_a[n_a], match_b[n_b], the pairs, the rounds run
// Every block is copied into buffers sized exactly, so an access past a row, a block or a match array
// is a sanitizer report. Prints "ok <records>" and exits 0, or a message and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ngs_match.h"

static int fail(const char* what, size_t i) {
    std::fprintf(stderr, "match_driver: %s at record %zu\n", what, i);
    return 1;
}

template <class T>
static bool get(std::FILE* in, std::vector<T>& v, size_t n) {
    v.assign(n, T());
    v.shrink_to_fit();
    return !n || std::fread(v.data(), sizeof(T), n, in) == n;
}
template <class T>
static bool put(std::FILE* out, const std::vector<T>& v) {
    return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), out) == v.size();
}
template <class T>
static std::vector<T> slice(const std::vector<T>& v, size_t a, size_t b) {
    std::vector<T> s(v.begin() + a, v.begin() + b);
    s.shrink_to_fit();
    return s;
}

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: match_driver IN OUT", 0);
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return fail("cannot open the files", 0);
    size_t rec = 0;
    uint32_t tag = 0;
    for (; std::fread(&tag, sizeof tag, 1, in) == 1; ++rec) {
        if (tag != 1 && tag != 2) return fail("unknown tag", rec);
        std::vector<uint32_t> h, cut, counts, keys;
        std::vector<float> values;
        if (!get(in, h, tag == 1 ? 5 : 6)) return fail("short input", rec);
        const uint32_t n_a = h[0], n_b = h[1], n = h[2], stride = h[3], first = h[4];
        if (tag == 2 && !get(in, cut, (size_t)h[5] + 1)) return fail("short input", rec);
        if (!get(in, counts, n) || !get(in, keys, (size_t)n * stride) || !get(in, values, (size_t)n * stride))
            return fail("short input", rec);
        std::vector<uint32_t> ma(n_a, ngs::kNoMatch), mb(n_b, ngs::kNoMatch);
        ma.shrink_to_fit();
        mb.shrink_to_fit();
        std::vector<uint32_t> tail;
        if (tag == 1) {
            tail.push_back(ngs::match_greedy(counts.data(), keys.data(), values.data(), n, stride, first, ma.data(), n_a,
                                             mb.data(), n_b));
        } else {
            if (cut.front() != 0 || cut.back() != n) return fail("bad cuts", rec);
            std::vector<uint64_t> bids(n_b, ~0ull);  // (BEGIN clears them)
            bids.shrink_to_fit();
            struct Block {
                std::vector<uint32_t> counts, keys;
                std::vector<float> values;
                uint32_t n, first;
            };
            std::vector<Block> blocks;
            for (size_t j = 0; j + 1 < cut.size(); ++j) {
                if (cut[j] > cut[j + 1]) return fail("bad cuts", rec);
                blocks.push_back({slice(counts, cut[j], cut[j + 1]),
                                  slice(keys, (size_t)cut[j] * stride, (size_t)cut[j + 1] * stride),
                                  slice(values, (size_t)cut[j] * stride, (size_t)cut[j + 1] * stride),
                                  cut[j + 1] - cut[j], first + cut[j]});
            }
            uint32_t pairs = 0, rounds = 0;
            for (;;) {
                uint32_t added = 0;
                for (size_t j = 0; j < blocks.size(); ++j) {
                    const Block& b = blocks[j];
                    ngs::match_round(b.counts.data(), b.keys.data(), b.values.data(), b.n, stride, b.first, ma.data(), n_a,
                                     mb.data(), n_b, bids.data(), (j == 0 ? ngs::kMatchBegin : 0u) | ngs::kMatchBid);
                }
                for (const Block& b : blocks)
                    added += ngs::match_round(b.counts.data(), b.keys.data(), b.values.data(), b.n, stride, b.first,
                                              ma.data(), n_a, mb.data(), n_b, bids.data(), ngs::kMatchAccept);
                ++rounds;
                pairs += added;
                if (!added) break;
                if (rounds > n_a + 1u) return fail("the rounds do not end", rec);
            }
            tail.push_back(pairs);
            tail.push_back(rounds);
        }
        for (uint32_t a = 0; a < n_a; ++a)
            if (ma[a] != ngs::kNoMatch && (ma[a] >= n_b || mb[ma[a]] != a)) return fail("the two sides disagree", rec);
        if (!put(out, ma) || !put(out, mb) || !put(out, tail)) return fail("cannot write", rec);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write", rec);
    std::printf("ok %zu\n", rec);
    return 0;
}
