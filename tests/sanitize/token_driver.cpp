// Drives the host token sort (stringsearchlib_amd/csrc/ngs_token.h: token_sort, the raw and the
// stored form, narrow and wide) for tests/test_token_host.py, built with g++ alone
// (-fsanitize=address,undefined).
//
//   token_driver IN OUT
// IN:  8 x u32 validChar set, u32 count, then per string u8 character size (1 or 4), u8 stored (0 / 1),
//      u32 length in characters, the characters.
// OUT: per string u32 length written, the characters: token_sort's output out of place.
// Every string is also sorted in place and by a brute-force sort of the split (tokens as vectors of
// their normalised characters, insertion sort); a difference between the three is an error here.
// Every buffer is sized exactly, so a read or write past a string is a sanitizer report.
// Prints "ok <strings>" and exits 0, or a message and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "ngs_token.h"

static int fail(const char* what, size_t i) {
    std::fprintf(stderr, "token_driver: %s at string %zu\n", what, i);
    return 1;
}

template <class CharT>
static std::vector<CharT> brute(const uint32_t* valid, const std::vector<CharT>& s, uint32_t cs, bool stored) {
    auto sep = [&](CharT c) { return stored ? ngs::sim_space(c) : !ngs::sim_keeps(valid, c, cs); };
    if (!stored && s.size() == 1 && s[0] == (CharT)'*') return s;
    std::vector<std::pair<std::vector<uint32_t>, std::vector<CharT>>> tokens;  // (normalised, raw)
    size_t first = s.size(), last = 0;
    for (size_t i = 0; i < s.size(); ++i) {
        if (sep(s[i])) continue;
        if (first == s.size()) first = i;
        last = i;
        if (i == 0 || sep(s[i - 1])) tokens.emplace_back();
        tokens.back().first.push_back(stored ? (uint32_t)s[i] : ngs::sim_norm(valid, s[i], cs));
        tokens.back().second.push_back(s[i]);
    }
    if (!tokens.empty() && last - first + 1 > ngs::kSimMaxQuery) return s;
    for (size_t i = 1; i < tokens.size(); ++i)  // insertion sort: an equal token stays behind its elders
        for (size_t j = i; j > 0 && tokens[j].first < tokens[j - 1].first; --j) std::swap(tokens[j], tokens[j - 1]);
    std::vector<CharT> out;
    for (size_t t = 0; t < tokens.size(); ++t) {
        if (t) out.push_back((CharT)' ');
        out.insert(out.end(), tokens[t].second.begin(), tokens[t].second.end());
    }
    if (!stored) out.resize(s.size(), (CharT)' ');
    return out;
}

template <class CharT>
static int one(std::FILE* in, std::FILE* out, const uint32_t* valid, uint32_t n, bool stored, size_t at) {
    std::vector<CharT> s(n);
    s.shrink_to_fit();  // exactly the string
    if (n && std::fread(s.data(), sizeof(CharT), n, in) != n) return fail("short input", at);
    const std::vector<CharT> want = brute(valid, s, (uint32_t)sizeof(CharT), stored);
    std::vector<CharT> got(stored ? want.size() : (size_t)n);  // exactly the output
    got.shrink_to_fit();
    const uint64_t len = ngs::token_sort(valid, s.data(), (uint64_t)n, (uint32_t)sizeof(CharT), stored, got.data());
    if (len != want.size() || got != want) return fail("token_sort differs from the brute-force sort", at);
    std::vector<CharT> place = s;
    const uint64_t len2 = ngs::token_sort(valid, place.data(), (uint64_t)n, (uint32_t)sizeof(CharT), stored, place.data());
    place.resize((size_t)len2);
    if (place != want) return fail("token_sort in place differs", at);
    const uint32_t l32 = (uint32_t)len;
    if (std::fwrite(&l32, sizeof l32, 1, out) != 1 ||
        (l32 && std::fwrite(got.data(), sizeof(CharT), l32, out) != l32))
        return fail("cannot write", at);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: token_driver IN OUT", 0);
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return fail("cannot open the files", 0);
    uint32_t valid[8], count = 0;
    if (std::fread(valid, sizeof valid, 1, in) != 1 || std::fread(&count, sizeof count, 1, in) != 1)
        return fail("short input", 0);
    for (size_t p = 0; p < count; ++p) {
        uint8_t head[2];
        uint32_t n = 0;
        if (std::fread(head, 1, 2, in) != 2 || std::fread(&n, sizeof n, 1, in) != 1) return fail("short input", p);
        if (head[0] != 1 && head[0] != 4) return fail("bad character size", p);
        const int rc = head[0] == 4 ? one<uint32_t>(in, out, valid, n, head[1] != 0, p)
                                    : one<uint8_t>(in, out, valid, n, head[1] != 0, p);
        if (rc) return rc;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write", count);
    std::printf("ok %u\n", count);
    return 0;
}
