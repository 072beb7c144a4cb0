// Drives the host routines of the edit-distance similarity (stringsearchlib_amd/csrc/ngs_sim.h)
// for tests/test_sim_host.py, built with g++ alone (-fsanitize=address,undefined).
//
//   sim_driver IN OUT
// IN:  u32 count, 8 x u32 validChar set, then per pair u16 raw query length + bytes, u16 term
//      length + bytes (the term as the index would store it).
// OUT: per pair 4 x u32: d and the bits of sim from the one-word routine (lev_myers64; 0xFFFFFFFF
//      and 0 when m > 64), d and the bits of sim from the multi-word routine (lev_myers_blocks).
//      A wildcard query writes 0xFFFFFFFF and the bits of kSimWildcard twice.
// The query is normalised here with the header's rules (sim_wildcard, sim_trim, sim_norm). Every
// buffer is sized exactly, so a read past a string is a sanitizer report.
// Prints "ok <pairs>" and exits 0, or a message and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ngs_sim.h"

static int fail(const char* what, size_t i) {
    std::fprintf(stderr, "sim_driver: %s at pair %zu\n", what, i);
    return 1;
}

static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, sizeof b);
    return b;
}

static bool read_string(std::FILE* in, std::vector<uint8_t>& s) {
    uint16_t len = 0;
    if (std::fread(&len, sizeof len, 1, in) != 1) return false;
    s.assign(len, 0);  // exactly the string
    s.shrink_to_fit();
    return !len || std::fread(s.data(), 1, len, in) == len;
}

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: sim_driver IN OUT", 0);
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return fail("cannot open the files", 0);
    uint32_t count = 0, valid[8];
    if (std::fread(&count, sizeof count, 1, in) != 1 || std::fread(valid, sizeof valid, 1, in) != 1)
        return fail("short input", 0);
    for (size_t p = 0; p < count; ++p) {
        std::vector<uint8_t> raw, term;
        if (!read_string(in, raw) || !read_string(in, term)) return fail("short input", p);
        const uint32_t L = (uint32_t)term.size();
        auto raw_at = [&](uint64_t i) { return (uint32_t)raw[i]; };
        auto t = [&](uint32_t j) { return (uint32_t)term[j]; };
        uint32_t res[4];
        if (ngs::sim_wildcard(raw_at, raw.size())) {
            res[0] = res[2] = 0xFFFFFFFFu;
            res[1] = res[3] = bits(ngs::kSimWildcard);
        } else {
            uint64_t first = 0;
            const uint32_t m = (uint32_t)ngs::sim_trim(valid, raw_at, raw.size(), 1, first);
            std::vector<uint32_t> Q(m);
            for (uint32_t i = 0; i < m; ++i) Q[i] = ngs::sim_norm(valid, raw[first + i], 1);
            auto q = [&](uint32_t i) { return Q.at(i); };
            res[0] = 0xFFFFFFFFu;
            res[1] = 0;
            if (m <= 64) {
                res[0] = ngs::lev_myers64(q, m, t, L);
                res[1] = bits(ngs::sim_value(res[0], m, L));
            }
            res[2] = ngs::lev_myers_blocks(q, m, t, L);
            res[3] = bits(ngs::sim_value(res[2], m, L));
        }
        if (std::fwrite(res, sizeof res, 1, out) != 1) return fail("cannot write", p);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write", count);
    std::printf("ok %u\n", count);
    return 0;
}
