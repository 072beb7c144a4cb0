// Drives the host routines of the similarity's metrics (stringsearchlib_amd/csrc/ngs_sim.h: OSA and
// PARTIAL, one word and multi-word) for tests/test_metric_host.py, built with g++ alone
// (-fsanitize=address,undefined).
//
//   metric_driver IN OUT
// IN:  u32 count, then per pair u16 query length + bytes, u16 term length + bytes. Both strings are
//      taken as they are: Q and T already normalised (sim_driver covers the normalisation).
// OUT: per pair 8 x u32: d and the bits of sim from osa_myers64 (0xFFFFFFFF and 0 when m > 64), from
//      osa_myers_blocks, from partial_myers64 (likewise) and from partial_myers_blocks.
// Every buffer is sized exactly, so a read past a string is a sanitizer report.
// Prints "ok <pairs>" and exits 0, or a message and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ngs_sim.h"

static int fail(const char* what, size_t i) {
    std::fprintf(stderr, "metric_driver: %s at pair %zu\n", what, i);
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
    if (argc != 3) return fail("usage: metric_driver IN OUT", 0);
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return fail("cannot open the files", 0);
    uint32_t count = 0;
    if (std::fread(&count, sizeof count, 1, in) != 1) return fail("short input", 0);
    for (size_t p = 0; p < count; ++p) {
        std::vector<uint8_t> Q, T;
        if (!read_string(in, Q) || !read_string(in, T)) return fail("short input", p);
        const uint32_t m = (uint32_t)Q.size(), L = (uint32_t)T.size();
        auto q = [&](uint32_t i) { return (uint32_t)Q.at(i); };
        auto t = [&](uint32_t j) { return (uint32_t)T.at(j); };
        uint32_t res[8] = {0xFFFFFFFFu, 0, 0, 0, 0xFFFFFFFFu, 0, 0, 0};
        if (m <= 64) {
            res[0] = ngs::osa_myers64(q, m, t, L);
            res[1] = bits(ngs::sim_value_metric(ngs::kSimOsa, res[0], m, L));
            res[4] = ngs::partial_myers64(q, m, t, L);
            res[5] = bits(ngs::sim_value_metric(ngs::kSimPartial, res[4], m, L));
        }
        res[2] = ngs::osa_myers_blocks(q, m, t, L);
        res[3] = bits(ngs::sim_value(res[2], m, L));
        res[6] = ngs::partial_myers_blocks(q, m, t, L);
        res[7] = bits(ngs::sim_value_partial(res[6], m));
        if (std::fwrite(res, sizeof res, 1, out) != 1) return fail("cannot write", p);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write", count);
    std::printf("ok %u\n", count);
    return 0;
}
