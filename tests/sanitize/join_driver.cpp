// Drives the host routines of the self-join (stringsearchlib_amd/csrc/ngs_join.h) for
// tests/test_join_host.py, built with g++ alone (-fsanitize=address,undefined).
//
//   join_driver IN OUT
// IN is a sequence of records, each a u32 tag and its fields (u32 unless said otherwise):
//   1 offsets  keys, first, n, cs, then u64 key_off[keys + 1]
//              -> OUT: u64 join_query_off(.., i, cs) for i = 0 .. n
//   2 drop     count, stride, self, limit, then keys[stride], f32 scores[stride]
//              -> OUT: the new count, keys[stride], scores[stride] (the row as drop_self_row left it)
//   3 cluster  flags, n_labels, n, stride, first, then counts[n], keys[n * stride]
//              flags 1: the labels start as k -> k; 2: finished and written -> OUT: labels[n_labels].
//              The forest lives from a record with flag 1 to the next one.
// Every buffer is sized exactly, so an access past a row or a label array is a sanitizer report.
// Prints "ok <records>" and exits 0, or a message and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ngs_join.h"

static int fail(const char* what, size_t i) {
    std::fprintf(stderr, "join_driver: %s at record %zu\n", what, i);
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

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: join_driver IN OUT", 0);
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return fail("cannot open the files", 0);
    std::vector<uint32_t> parent;
    size_t rec = 0;
    uint32_t tag = 0;
    for (; std::fread(&tag, sizeof tag, 1, in) == 1; ++rec) {
        std::vector<uint32_t> h;
        if (tag == 1) {
            std::vector<uint64_t> key_off, res;
            if (!get(in, h, 4) || !get(in, key_off, (size_t)h[0] + 1)) return fail("short input", rec);
            for (uint32_t i = 0; i <= h[2]; ++i) res.push_back(ngs::join_query_off(key_off.data(), h[1], i, h[3]));
            if (!put(out, res)) return fail("cannot write", rec);
        } else if (tag == 2) {
            std::vector<uint32_t> keys;
            std::vector<float> scores;
            if (!get(in, h, 4) || !get(in, keys, h[1]) || !get(in, scores, h[1])) return fail("short input", rec);
            const std::vector<uint32_t> kept{ngs::drop_self_row(keys.data(), scores.data(), h[0], h[1], h[2], h[3])};
            if (!put(out, kept) || !put(out, keys) || !put(out, scores)) return fail("cannot write", rec);
        } else if (tag == 3) {
            std::vector<uint32_t> counts, keys;
            if (!get(in, h, 5) || !get(in, counts, h[2]) || !get(in, keys, (size_t)h[2] * h[3]))
                return fail("short input", rec);
            if (h[0] & ngs::kClusterInit) {
                parent.assign(h[1], 0);
                parent.shrink_to_fit();
                for (uint32_t k = 0; k < h[1]; ++k) parent[k] = k;
            }
            if (parent.size() != h[1]) return fail("label count changed", rec);
            ngs::uf_block(parent.data(), h[1], counts.data(), keys.data(), h[2], h[3], h[4]);
            for (uint32_t k = 0; k < h[1]; ++k)
                if (parent[k] > k) return fail("parent above its node", rec);
            if (h[0] & ngs::kClusterFinish) {
                ngs::uf_finish(parent.data(), h[1]);
                if (!put(out, parent)) return fail("cannot write", rec);
            }
        } else {
            return fail("unknown tag", rec);
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write", rec);
    std::printf("ok %zu\n", rec);
    return 0;
}
