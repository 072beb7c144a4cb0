// Drives the host UTF-8 codec (stringsearchlib_amd/csrc/ngs_utf8.h) for tests/test_utf8_host.py,
// built with g++ alone (plain and -fsanitize=address,undefined).
//
//   utf8_driver IN OUT
// IN:  u32 count, then per string u8 length + bytes.   OUT: per string u32 units + the units.
// Besides decoding, every string is checked here: the decoder's count-only form agrees, the
// per-byte rule (utf8_starts, what the device kernels run) marks exactly the unit starts the
// sequential decoder takes, utf8_encoded_len matches what utf8_encode writes, and
// encode(decode(s)) == s. Every buffer is sized exactly, so an overrun is a sanitizer report.
// Prints "ok <strings> <units>" and exits 0, or a message and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ngs_utf8.h"

static int fail(const char* what, size_t i) {
    std::fprintf(stderr, "utf8_driver: %s at string %zu\n", what, i);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: utf8_driver IN OUT", 0);
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return fail("cannot open the files", 0);
    uint32_t count = 0;
    if (std::fread(&count, sizeof count, 1, in) != 1) return fail("short input", 0);
    uint64_t total = 0;
    for (size_t i = 0; i < count; ++i) {
        uint8_t len = 0;
        if (std::fread(&len, 1, 1, in) != 1) return fail("short input", i);
        std::vector<uint8_t> s(len);  // exactly the string: reads past it are reported
        if (len && std::fread(s.data(), 1, len, in) != len) return fail("short input", i);
        const size_t n_units = ngs::utf8_decode(s.data(), len, nullptr);
        std::vector<uint32_t> units(n_units);
        if (ngs::utf8_decode(s.data(), len, units.data()) != n_units) return fail("count-only form differs", i);
        // the per-byte rule against the sequential walk
        std::vector<char> starts(len, 0);
        for (size_t p = 0; p < len;) {
            starts[p] = 1;
            const uint32_t wf = ngs::utf8_wf_len(s.data() + p, len - p);
            p += wf ? wf : 1;
        }
        for (size_t p = 0; p < len; ++p)
            if (ngs::utf8_starts(s.data(), len, p) != (starts[p] != 0)) return fail("per-byte rule differs", i);
        // the inverse
        const size_t enc_len = ngs::utf8_encoded_len(units.data(), n_units);
        if (enc_len != len) return fail("utf8_encoded_len differs from the source length", i);
        std::vector<uint8_t> back(enc_len);
        if (ngs::utf8_encode(units.data(), n_units, back.data()) != enc_len) return fail("utf8_encode length", i);
        if (len && std::memcmp(back.data(), s.data(), len) != 0) return fail("round trip differs", i);
        const uint32_t nu = (uint32_t)n_units;
        if (std::fwrite(&nu, sizeof nu, 1, out) != 1 ||
            (n_units && std::fwrite(units.data(), sizeof(uint32_t), n_units, out) != n_units))
            return fail("cannot write", i);
        total += n_units;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write", count);
    std::printf("ok %u %llu\n", count, (unsigned long long)total);
    return 0;
}
