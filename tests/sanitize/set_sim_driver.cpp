// set_sim_driver — the host reference routines of the similarity over an index set (ngs_set.h:
// sim_set_part, sim_set_record) in a stand-alone program, for tests/test_set_sim_host.py:
//   g++ -std=c++17 -fsanitize=address,undefined -I stringsearchlib_amd/csrc set_sim_driver.cpp
//   set_sim_driver in.bin out.bin
// in.bin, little-endian u32 words, one record after another until the end of the file:
//   P, G, then per member: form (0: kt_off / kt_term, 1: key_term), n_keys, n_terms, base, and
//   form 0: kt_off[n_keys + 1], kt_term[kt_off[n_keys]]; form 1: key_term[n_keys];
//   then the G global key ids.
// out.bin, per id: part (0xFFFFFFFF none), local key, the number of term ids, the term ids.
// Every array lives in a vector of its exact size, so a read past one is an ASan report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ngs_set.h"

namespace {
bool read_words(std::FILE* f, std::vector<uint32_t>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(uint32_t), n, f) == n;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    unsigned records = 0;
    for (;;) {
        uint32_t head[2];
        if (std::fread(head, sizeof(uint32_t), 2, in) != 2) break;
        const uint32_t P = head[0], G = head[1];
        if (P > ngs::kSetMaxParts) return 3;
        std::vector<ngs::SimMember> m(P);
        std::vector<std::vector<uint32_t>> off(P), term(P), key_term(P);
        for (uint32_t p = 0; p < P; ++p) {
            uint32_t h[4];
            if (std::fread(h, sizeof(uint32_t), 4, in) != 4) return 3;
            m[p] = ngs::SimMember{nullptr, nullptr, nullptr, nullptr, nullptr, h[1], h[2], h[3], 0u};
            if (h[0] == 0) {
                if (!read_words(in, off[p], (size_t)h[1] + 1) || !read_words(in, term[p], off[p][h[1]])) return 3;
                m[p].kt_off = off[p].data();
                m[p].kt_term = term[p].data();
            } else {
                if (!read_words(in, key_term[p], h[1])) return 3;
                m[p].key_term = key_term[p].data();
            }
        }
        std::vector<uint32_t> ids;
        if (!read_words(in, ids, G)) return 3;
        for (uint32_t g : ids) {
            uint32_t p = 0, key = 0, n = 0;
            std::vector<uint32_t> terms(8);
            const bool owned = ngs::sim_set_record(m.data(), P, g, p, key, terms.data(), (uint32_t)terms.size(), n);
            if (owned && n > terms.size()) {  // the count first, then room for all of them
                terms.resize(n);
                ngs::sim_set_record(m.data(), P, g, p, key, terms.data(), n, n);
            }
            if (owned != (p != ngs::kSetNoPart) || (owned && p != ngs::sim_set_part(m.data(), P, g))) return 4;
            const uint32_t row[3] = {p, owned ? key : 0u, n};
            std::fwrite(row, sizeof(uint32_t), 3, out);
            if (n) std::fwrite(terms.data(), sizeof(uint32_t), n, out);
        }
        ++records;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("ok %u\n", records);
    return 0;
}
