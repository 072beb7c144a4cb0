// ngs_sim.h — the edit-distance similarity behind the search: one definition
// shared by the host reference routines and the device kernels (ngs_sim.hip).
//
// A record is (query, key). Q is the query normalised as k_prep does it (every character through
// escapeBlank with the handle's validChar set, blanks trimmed at both ends, then toupper; m = |Q|),
// T a normalised term of the key as the index stores it (L = |T| >= 1). d(Q, T) is the unit-cost
// Levenshtein distance (global: both ends fixed) and
//     sim(Q, T) = 1.0f - (float)d / (float)max(m, L)
// in fp32: one correctly rounded division and one subtraction, never contracted, so
// numpy.float32 arithmetic gives the same bits. A record's similarity is the largest over the
// key's terms. Wildcard queries score kSimWildcard on every record; a query of more than
// kSimMaxQuery characters, or a key id outside the index, kSimNone ("not computed").
//
// A metric selects d and the divisor: kSimLevenshtein is the above, and what the
// entry points without a metric compute; kSimOsa adds the adjacent transposition at cost 1
// (optimal string alignment: no substring is edited twice), same divisor; kSimPartial is the
// semi-global form, d = the least Levenshtein distance of Q to any substring of T (the empty one
// included, so d <= m), sim = 1 - d / m for m >= 1 and 0 for m = 0. The matched term is the term id
// that attains a record's similarity, the smallest such id; kSimNoTerm where no term was compared.
//
// Plain C++17 without a HIP include: g++ compiles the host routines alone (tests/sanitize).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "ngs_common.h"
#define NGS_HD __host__ __device__
#else
#define NGS_HD
#endif

namespace ngs {

constexpr uint32_t kSimMaxQuery = 4096;     // normalised query characters the kernels take
constexpr uint32_t kRerankMaxStride = 4096; // records per query ngsRerankDevice sorts (LDS: 8 bytes each)
constexpr float kSimWildcard = 1.0f;
constexpr float kSimNone = -1.0f;
constexpr uint32_t kSimLevenshtein = 0, kSimOsa = 1, kSimPartial = 2;  // NGS_SIM_* of the public header
constexpr uint32_t kSimMetrics = 3;
constexpr uint32_t kSimNoTerm = 0xFFFFFFFFu;  // "no term was compared"

// ---- normalisation of one character (the one-liners of ngs_kernels.hip, restated) ----
NGS_HD inline bool sim_space(uint32_t c) { return c == 32u || (c >= 9u && c <= 13u); }
NGS_HD inline uint32_t sim_upper(uint32_t c) { return (c >= 'a' && c <= 'z') ? c - 32u : c; }
// escapeBlank: a byte (cs 1) or a wide character below 128 outside the 256-bit validChar set
// becomes a space; wide characters from 128 are kept, non-code-points (> 0x10FFFF) become spaces
NGS_HD inline uint32_t sim_esc(const uint32_t* valid, uint32_t c, uint32_t cs) {
    if (cs == 1 || c < 128u) return ((valid[(c & 255u) >> 5] >> (c & 31u)) & 1u) ? c : 32u;
    return c > 0x10FFFFu ? 32u : c;
}
// a character kept by the trim: not blank after the escape
NGS_HD inline bool sim_keeps(const uint32_t* valid, uint32_t c, uint32_t cs) { return !sim_space(sim_esc(valid, c, cs)); }
// the character as Q holds it
NGS_HD inline uint32_t sim_norm(const uint32_t* valid, uint32_t c, uint32_t cs) { return sim_upper(sim_esc(valid, c, cs)); }

// Wildcard rule (nGramSearch.hpp:356): the raw query is empty or the single character '*'.
template <class CharAt>
NGS_HD inline bool sim_wildcard(CharAt raw, uint64_t n) {
    return n == 0 || (n == 1 && raw(0) == (uint32_t)'*');
}

// Trim rule: Q is raw[first .. first + m) normalised, where first / first + m - 1 are the first
// and last characters the trim keeps; m = 0 when none is kept (Q is empty, d = L, sim = 0).
template <class CharAt>
NGS_HD inline uint64_t sim_trim(const uint32_t* valid, CharAt raw, uint64_t n, uint32_t cs, uint64_t& first) {
    uint64_t a = 0, e = n;
    while (a < e && !sim_keeps(valid, raw(a), cs)) ++a;
    while (e > a && !sim_keeps(valid, raw(e - 1), cs)) --e;
    first = a;
    return e - a;
}

// ---- Myers' bit-vector algorithm, global form (Hyyro's block step) ----
// One 64-row block of the DP column: pv / mv hold the vertical deltas (+1 / -1) of its rows, eq the
// rows whose query character equals the column's term character, hin (-1, 0, +1) the horizontal
// delta entering the block's first row, `top` the bit of the row whose horizontal delta is
// returned (the block's last row: bit 63, or (m - 1) % 64 in the query's last block; rows above
// it in that block hold nothing that reaches lower rows). Row 0 of the whole column has horizontal
// delta +1 (the top boundary D[0][j] = j): the first block is stepped with hin = +1. This is what
// tells it from the approximate-matching form of myers_match_t, whose row 0 delta is 0.
struct MyersBlock {
    uint64_t pv = ~0ull, mv = 0;  // D[i][0] = i: every vertical delta is +1
};
NGS_HD inline int myers_step(MyersBlock& b, uint64_t eq, int hin, uint64_t top) {
    const uint64_t neg = hin < 0 ? 1ull : 0ull;
    const uint64_t xv = eq | b.mv;
    eq |= neg;
    const uint64_t xh = (((eq & b.pv) + b.pv) ^ b.pv) | eq;
    uint64_t ph = b.mv | ~(xh | b.pv);
    uint64_t mh = b.pv & xh;
    const int hout = (ph & top) ? 1 : ((mh & top) ? -1 : 0);
    ph = (ph << 1) | (hin > 0 ? 1ull : 0ull);
    mh = (mh << 1) | neg;
    b.pv = mh | ~(xv | ph);
    b.mv = ph & xv;
    return hout;
}

// The same block with the adjacent transposition (Hyyro's OSA extension). d0: the rows of the
// previous column whose diagonal delta was 0; eqp: the previous column's eq. A row i may take the
// transposition when Q_i = T_{j-1} (eqp), Q_{i-1} = T_j (eq, one row up) and D[i-1][j-1] was not
// reached by a zero diagonal (~d0, one row up). The row above a block's first row is the last row
// of the block above: its bit comes in as tin and this block's bit 63 goes out as tout (0 / 1),
// beside hin / hout. The first block takes tin = 0.
struct OsaBlock : MyersBlock {
    uint64_t d0 = 0, eqp = 0;
};
NGS_HD inline int osa_step(OsaBlock& b, uint64_t eq, int hin, uint32_t tin, uint64_t top, uint32_t& tout) {
    const uint64_t neg = hin < 0 ? 1ull : 0ull;
    uint64_t xv = eq | b.mv;
    const uint64_t eqn = eq | neg;
    uint64_t xh = (((eqn & b.pv) + b.pv) ^ b.pv) | eqn;
    const uint64_t x = ~b.d0 & eq;
    const uint64_t tr = ((x << 1) | (uint64_t)tin) & b.eqp;
    xh |= tr;
    xv |= tr;
    tout = (uint32_t)(x >> 63);
    b.d0 = xh | b.mv;
    b.eqp = eq;
    uint64_t ph = b.mv | ~(xh | b.pv);
    uint64_t mh = b.pv & xh;
    const int hout = (ph & top) ? 1 : ((mh & top) ? -1 : 0);
    ph = (ph << 1) | (hin > 0 ? 1ull : 0ull);
    mh = (mh << 1) | neg;
    b.pv = mh | ~(xv | ph);
    b.mv = ph & xv;
    return hout;
}

// the fp32 similarity of a distance
NGS_HD inline float sim_value(uint32_t d, uint32_t m, uint32_t L) {
    const uint32_t mx = m > L ? m : L;
    if (mx == 0) return 1.0f;  // (no term is empty; two empty strings are equal)
    return 1.0f - (float)d / (float)mx;
}
// ... of kSimPartial's distance: the divisor is the query's length
NGS_HD inline float sim_value_partial(uint32_t d, uint32_t m) {
    if (m == 0) return 0.0f;
    return 1.0f - (float)d / (float)m;
}
NGS_HD inline float sim_value_metric(uint32_t metric, uint32_t d, uint32_t m, uint32_t L) {
    return metric == kSimPartial ? sim_value_partial(d, m) : sim_value(d, m, L);
}

// ---- host reference routines (the device kernels restate them over LDS tables) ----
// d(Q, T) for m <= 64 with one word. q / t: accessors of the normalised characters.
template <class QF, class TF>
inline uint32_t lev_myers64(QF q, uint32_t m, TF t, uint32_t L) {
    if (m == 0) return L;
    const uint64_t top = 1ull << (m - 1u);
    MyersBlock b;
    uint32_t score = m;
    for (uint32_t j = 0; j < L; ++j) {
        const uint32_t c = t(j);
        uint64_t eq = 0;
        for (uint32_t i = 0; i < m; ++i) eq |= q(i) == c ? 1ull << i : 0ull;
        score += (uint32_t)myers_step(b, eq, +1, top);
    }
    return score;
}

// d(Q, T) for any m <= kSimMaxQuery with ceil(m / 64) words, the horizontal delta carried from
// block to block within a column (the systolic kernel carries it from lane to lane instead).
template <class QF, class TF>
inline uint32_t lev_myers_blocks(QF q, uint32_t m, TF t, uint32_t L) {
    if (m == 0) return L;
    if (m > kSimMaxQuery) return 0xFFFFFFFFu;
    const uint32_t W = (m + 63u) / 64u;
    MyersBlock blk[kSimMaxQuery / 64];
    uint32_t score = m;
    for (uint32_t j = 0; j < L; ++j) {
        const uint32_t c = t(j);
        int h = +1;
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t rows = w + 1 < W ? 64u : m - 64u * w;
            uint64_t eq = 0;
            for (uint32_t i = 0; i < rows; ++i) eq |= q(64u * w + i) == c ? 1ull << i : 0ull;
            h = myers_step(blk[w], eq, h, 1ull << (rows - 1u));
        }
        score += (uint32_t)h;
    }
    return score;
}

// the rows of query word w (of W) matching character c
template <class QF>
inline uint64_t sim_word_eq(QF q, uint32_t w, uint32_t rows, uint32_t c) {
    uint64_t eq = 0;
    for (uint32_t i = 0; i < rows; ++i) eq |= q(64u * w + i) == c ? 1ull << i : 0ull;
    return eq;
}

// kSimOsa's d(Q, T), one word (m <= 64)
template <class QF, class TF>
inline uint32_t osa_myers64(QF q, uint32_t m, TF t, uint32_t L) {
    if (m == 0) return L;
    const uint64_t top = 1ull << (m - 1u);
    OsaBlock b;
    uint32_t score = m, tout = 0;
    for (uint32_t j = 0; j < L; ++j) score += (uint32_t)osa_step(b, sim_word_eq(q, 0, m, t(j)), +1, 0u, top, tout);
    return score;
}

// ... any m <= kSimMaxQuery: hout and tout carried from block to block within a column
template <class QF, class TF>
inline uint32_t osa_myers_blocks(QF q, uint32_t m, TF t, uint32_t L) {
    if (m == 0) return L;
    if (m > kSimMaxQuery) return 0xFFFFFFFFu;
    const uint32_t W = (m + 63u) / 64u;
    OsaBlock blk[kSimMaxQuery / 64];
    uint32_t score = m;
    for (uint32_t j = 0; j < L; ++j) {
        const uint32_t c = t(j);
        int h = +1;
        uint32_t tr = 0;
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t rows = w + 1 < W ? 64u : m - 64u * w;
            h = osa_step(blk[w], sim_word_eq(q, w, rows, c), h, tr, 1ull << (rows - 1u), tr);
        }
        score += (uint32_t)h;
    }
    return score;
}

// kSimPartial's d(Q, T): row 0 of every column is 0 (hin = 0 into the first block), and d is the
// least of the last row over columns 0 .. L (column 0 holds m)
template <class QF, class TF>
inline uint32_t partial_myers64(QF q, uint32_t m, TF t, uint32_t L) {
    if (m == 0) return 0;
    const uint64_t top = 1ull << (m - 1u);
    MyersBlock b;
    uint32_t score = m, best = m;
    for (uint32_t j = 0; j < L; ++j) {
        score += (uint32_t)myers_step(b, sim_word_eq(q, 0, m, t(j)), 0, top);
        if (score < best) best = score;
    }
    return best;
}

template <class QF, class TF>
inline uint32_t partial_myers_blocks(QF q, uint32_t m, TF t, uint32_t L) {
    if (m == 0) return 0;
    if (m > kSimMaxQuery) return 0xFFFFFFFFu;
    const uint32_t W = (m + 63u) / 64u;
    MyersBlock blk[kSimMaxQuery / 64];
    uint32_t score = m, best = m;
    for (uint32_t j = 0; j < L; ++j) {
        const uint32_t c = t(j);
        int h = 0;
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t rows = w + 1 < W ? 64u : m - 64u * w;
            h = myers_step(blk[w], sim_word_eq(q, w, rows, c), h, 1ull << (rows - 1u));
        }
        score += (uint32_t)h;
        if (score < best) best = score;
    }
    return best;
}

// ---- the similarity's view of an index ----
// What the kernels read of one index: its key -> terms arrays (kt_off / kt_term, or key_term where
// every key has one pair: kt_off null) and its terms (term_off / term_bytes, or the token-sorted
// pair). `base` is the first key id the index owns: 0 for a single index, the member's base in an
// index set (ngs_set.h), whose members travel by value in the kernel arguments.
struct SimMember {
    const uint32_t* kt_off;
    const uint32_t* kt_term;
    const uint32_t* key_term;
    const uint64_t* term_off;
    const uint8_t* term_bytes;
    uint32_t n_keys, n_terms, base, pad;
};
static_assert(sizeof(SimMember) == 56, "16 members x 56 bytes travel in the kernel arguments");

// ---- the wide short path's match-mask table: open addressing over kSimSlots slots ----
constexpr uint32_t kSimSlots = 128;            // <= 64 distinct characters: at most half full
constexpr uint32_t kSimEmpty = 0xFFFFFFFFu;    // no normalised character (they are <= 0x10FFFF)
NGS_HD inline uint32_t sim_slot(uint32_t c) { return (c * 0x9E3779B1u) >> 25; }  // top 7 bits; probing is linear

// ---- ngsRerankDevice's sort key ----
// fp32 -> u32 whose unsigned order is the floats' order (no NaN occurs: sims are -1 or in [0, 1])
NGS_HD inline uint32_t sim_order_bits(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
// ascending key = (sim descending, position ascending); kRerankDropped sorts last
constexpr uint64_t kRerankDropped = ~0ull;
NGS_HD inline uint64_t rerank_key(uint32_t sim_bits, uint32_t pos) {
    return ((uint64_t)(~sim_order_bits(sim_bits)) << 32) | pos;
}

#if defined(__HIPCC__)
// dSim[i * stride + r], r < min(dCounts[i], stride): the similarity by `metric` (< kSimMetrics) of query i
// and key dKeys[i * stride + r]; with terms != null the matched term ids in sim's layout.
// key_term: term of each key (indexes without kt_off), else null. Queues on s; no host wait.
hipError_t launch_similarity(const DevIndex& X, const uint32_t valid[8], const uint32_t* key_term,
                             const uint8_t* raw, const uint64_t* off, uint32_t n, uint32_t stride,
                             const uint32_t* counts, const uint32_t* keys, uint32_t metric, float* sim,
                             uint32_t* terms, hipStream_t s);
// per query: records with sim < min_sim dropped, the rest ordered (sim desc, position asc), in place,
// the matched terms (may be null) permuted with them
hipError_t launch_rerank(uint32_t n, uint32_t stride, uint32_t* counts, uint32_t* keys, float* scores, float* sim,
                         uint32_t* terms, float min_sim, hipStream_t s);
// key_term[k] = the term of key k's pair (kSimEmpty: none) of an index whose keys have one pair each
hipError_t build_key_term(const DevIndex& X, uint32_t* key_term, hipStream_t s);
#endif

}  // namespace ngs
