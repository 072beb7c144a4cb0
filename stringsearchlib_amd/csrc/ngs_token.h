// ngs_token.h — the token sort in front of the similarity: one definition shared
// by the host routine below and the device kernel (ngs_token.hip).
//
// A string's characters c_0 .. c_{n-1} are split at its separators into tokens, the maximal runs of
// the other characters. In the raw form (a query as ngsSearchDevice takes it) a separator is a
// character the trim does not keep (!sim_keeps: blank after the escape) and tokens are compared by
// their normalised characters (sim_norm); in the stored form (a term as the index holds it: already
// normalised) a separator is sim_space and the characters compare as they are. The tokens are
// ordered by those characters as unsigned values, lexicographically, a proper prefix first, equal
// tokens in their order of appearance (the sort is stable). The output is the tokens' characters as
// they came in that order, one ' ' between neighbours: the raw form is then filled with ' ' up
// to n (the length is kept, so the wildcard rule reads the same string lengths), the stored form
// ends there (its length L' <= n). A string with more than kSimMaxQuery characters between its
// first and last token character is copied unchanged (the similarity does not take it either), and
// so is the raw string "*": the wildcard rule reads the raw characters, and '*' need not be a
// character the validChar set keeps.
//
// Plain C++17 without a HIP include: g++ compiles the host routine alone (tests/sanitize).
#pragma once

#include <algorithm>
#include <vector>

#include "ngs_sim.h"

namespace ngs {

constexpr uint32_t kSimTokenSort = 0x100u;             // NGS_SIM_TOKEN_SORT of the public header
constexpr uint32_t kTokenMaxCount = kSimMaxQuery / 2;  // tokens of a span of kSimMaxQuery characters, at the most
// a metric with or without the flag; the base metric
NGS_HD inline bool sim_metric_ok(uint32_t metric) { return (metric & ~kSimTokenSort) < kSimMetrics; }
NGS_HD inline uint32_t sim_metric_base(uint32_t metric) { return metric & ~kSimTokenSort; }

// The host routine: in[0 .. n) -> out (n characters are written in the raw form, the returned L'
// in the stored form; out may be in). valid: the validChar set (raw form); cs: 1 or 4, as sim_esc
// takes it. Returns the characters written.
template <class CharT>
inline uint64_t token_sort(const uint32_t* valid, const CharT* in, uint64_t n, uint32_t cs, bool stored, CharT* out) {
    auto sep = [&](uint64_t i) { return stored ? sim_space((uint32_t)in[i]) : !sim_keeps(valid, (uint32_t)in[i], cs); };
    auto norm = [&](uint64_t i) { return stored ? (uint32_t)in[i] : sim_norm(valid, (uint32_t)in[i], cs); };
    uint64_t a = 0, e = n;
    while (a < e && sep(a)) ++a;
    while (e > a && sep(e - 1)) --e;
    if (e - a > kSimMaxQuery || (!stored && n == 1 && (uint32_t)in[0] == (uint32_t)'*')) {
        if (out != in) std::copy(in, in + n, out);
        return n;
    }
    struct Token {
        uint64_t start, len;
    };
    std::vector<Token> tokens;
    for (uint64_t i = a; i < e;) {
        if (sep(i)) {
            ++i;
            continue;
        }
        uint64_t j = i;
        while (j < e && !sep(j)) ++j;
        tokens.push_back({i, j - i});
        i = j;
    }
    std::stable_sort(tokens.begin(), tokens.end(), [&](const Token& x, const Token& y) {
        const uint64_t k = std::min(x.len, y.len);
        for (uint64_t i = 0; i < k; ++i) {
            const uint32_t cx = norm(x.start + i), cy = norm(y.start + i);
            if (cx != cy) return cx < cy;
        }
        return x.len < y.len;
    });
    std::vector<CharT> sorted;
    sorted.reserve((size_t)(e - a));
    for (size_t t = 0; t < tokens.size(); ++t) {
        if (t) sorted.push_back((CharT)' ');
        sorted.insert(sorted.end(), in + tokens[t].start, in + tokens[t].start + tokens[t].len);
    }
    std::copy(sorted.begin(), sorted.end(), out);
    if (stored) return sorted.size();
    std::fill(out + sorted.size(), out + n, (CharT)' ');
    return n;
}

#if defined(__HIPCC__)
// The raw form over a query batch: string i of raw[off[i] .. off[i + 1]) (bytes; characters of cs
// bytes) token-sorted into out at the same offsets; out may be raw. Queues on s; no host wait.
hipError_t launch_token_sort(const uint32_t valid[8], uint32_t cs, const uint8_t* raw, const uint64_t* off, uint32_t n,
                             uint8_t* out, hipStream_t s);
// The stored form over the index's terms, in two passes. Pass 1: ts_off[n_terms + 1] = the exclusive
// sums of the sorted terms' lengths L' (character offsets, as term_off holds them); synchronous on s
// (it takes and frees the scan's scratch). Pass 2: the sorted terms into ts_bytes at those offsets.
hipError_t sorted_term_offsets(const DevIndex& X, uint64_t* ts_off, hipStream_t s);
hipError_t launch_sorted_terms(const DevIndex& X, const uint64_t* ts_off, uint8_t* ts_bytes, hipStream_t s);
#endif

}  // namespace ngs
