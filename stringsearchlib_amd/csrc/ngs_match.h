// ngs_match.h — linking two indexes: the greedy one-to-one matching of source keys
// to target keys over a block of candidate records, shared by the host routines and the device
// kernels (ngs_match.hip).
//
// S is the source index (nS keys), T the target (nT keys). The candidate row of source key a is the
// answer ngsSearchDevice on T gives at (threshold, limit) for a's raw string, normalised with T's
// validChar set, no record dropped; Ls = min(limit, nT) is the row stride. With a similarity filter
// a record is kept unless its similarity (T's, by a metric) is below the bound, in the search's order.
// The value of a record is its similarity with the filter and its score without; an edge is
// (a, b, value). Edges are totally ordered by value descending, then a ascending, then b ascending;
// values compare by sim_order_bits of their fp32 bits (numeric order for non-NaN floats with
// -0 < +0; a NaN sorts where its bits put it).
//   best        match[a] = the b of a's first edge in that order (kNoMatch for an empty row);
//   one-to-one  the greedy matching: every edge in that order, taken iff both its ends are free.
//
// The block has ngsSearchDevice's layout: the edges of row i are (first + i, keys[i * stride + r],
// values[i * stride + r]), r < min(counts[i], stride). An edge with a >= nA or b >= nB is ignored.
//
// The parallel form is rounds. An edge is live when both its ends are unmatched. A round lets every
// live edge bid for its b (bids[b] = the largest live edge at b), then lets every unmatched row take
// its own largest live edge if that edge also holds the bid at its b. Edges that are largest at both
// ends are vertex-disjoint, and each is what the sequential pass takes next among the live edges, so
// the rounds build exactly the sequential matching; the largest live edge overall always wins, so
// a round with live edges matches at least one, and the first round that matches none ends it.
//
// Plain C++17 without a HIP include: g++ compiles the host routines alone (tests/sanitize).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ngs_sim.h"

namespace ngs {

constexpr uint32_t kNoMatch = 0xFFFFFFFFu;  // NGS_NO_MATCH
constexpr uint32_t kMatchInit = 1u, kMatchBegin = 2u, kMatchBid = 4u, kMatchAccept = 8u;  // NGS_MATCH_*
constexpr uint32_t kMatchFlags = kMatchInit | kMatchBegin | kMatchBid | kMatchAccept;
constexpr uint32_t kLinkBest = 0u, kLinkOneToOne = 1u;  // NGS_LINK_*
constexpr uint32_t kLinkModes = 2;

// The edge (a, b, value) as the two ends see it: larger = earlier in the edge order. At b the edges
// differ in (value, a), at a in (value, b); an id is < 0xFFFFFFFF, so a key is never 0 ("no edge").
NGS_HD inline uint64_t match_key(uint32_t value_bits, uint32_t other_end) {
    return ((uint64_t)sim_order_bits(value_bits) << 32) | (0xFFFFFFFFu - other_end);
}
NGS_HD inline uint32_t match_key_end(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// ---- host reference routines (the kernels restate them with a group of lanes per row) ----
inline uint32_t match_bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

// Row i's largest edge (as match_key(value, b)) among those with b < nB and, with match_b, a free
// b; 0 for none.
inline uint64_t match_row_best(const uint32_t* counts, const uint32_t* keys, const float* values, uint32_t i,
                               uint32_t stride, uint32_t n_b, const uint32_t* match_b) {
    const uint32_t c = counts[i] < stride ? counts[i] : stride;
    uint64_t best = 0;
    for (uint32_t r = 0; r < c; ++r) {
        const uint32_t b = keys[(size_t)i * stride + r];
        if (b >= n_b || (match_b && match_b[b] != kNoMatch)) continue;
        best = std::max(best, match_key(match_bits(values[(size_t)i * stride + r]), b));
    }
    return best;
}

// The sequential greedy over one block into match_a[n_a] / match_b[n_b] (both kNoMatch before the
// first block of a matching that is made of one block): every edge sorted, then one pass. Returns
// the pairs it added. A matching over several blocks needs their edges in one sort: concatenate.
inline uint32_t match_greedy(const uint32_t* counts, const uint32_t* keys, const float* values, uint32_t n,
                             uint32_t stride, uint32_t first, uint32_t* match_a, uint32_t n_a, uint32_t* match_b,
                             uint32_t n_b) {
    struct Edge {
        uint32_t order, a, b;
    };
    std::vector<Edge> edges;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t a = (uint64_t)first + i;
        const uint32_t c = counts[i] < stride ? counts[i] : stride;
        if (a >= n_a) continue;
        for (uint32_t r = 0; r < c; ++r) {
            const uint32_t b = keys[(size_t)i * stride + r];
            if (b < n_b) edges.push_back({sim_order_bits(match_bits(values[(size_t)i * stride + r])), (uint32_t)a, b});
        }
    }
    std::sort(edges.begin(), edges.end(), [](const Edge& x, const Edge& y) {
        if (x.order != y.order) return x.order > y.order;
        if (x.a != y.a) return x.a < y.a;
        return x.b < y.b;
    });
    uint32_t added = 0;
    for (const Edge& e : edges)
        if (match_a[e.a] == kNoMatch && match_b[e.b] == kNoMatch) {
            match_a[e.a] = e.b;
            match_b[e.b] = e.a;
            ++added;
        }
    return added;
}

// One step of a round over one block, as ngsMatchDevice's flags name them. BEGIN clears bids[n_b];
// BID raises bids[b] to the largest live edge of the block at b; ACCEPT lets every unmatched row of
// the block take its largest live edge if bids[] names that very edge, and returns the pairs added
// (the rows go in ascending order and see the matches of the rows before them, which is one of the
// orders the kernel's waves may run in).
inline uint32_t match_round(const uint32_t* counts, const uint32_t* keys, const float* values, uint32_t n,
                            uint32_t stride, uint32_t first, uint32_t* match_a, uint32_t n_a, uint32_t* match_b,
                            uint32_t n_b, uint64_t* bids, uint32_t flags) {
    if (flags & kMatchBegin) std::fill(bids, bids + n_b, (uint64_t)0);
    if (flags & kMatchBid)
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t a = (uint64_t)first + i;
            if (a >= n_a || match_a[a] != kNoMatch) continue;
            const uint32_t c = counts[i] < stride ? counts[i] : stride;
            for (uint32_t r = 0; r < c; ++r) {
                const uint32_t b = keys[(size_t)i * stride + r];
                if (b >= n_b || match_b[b] != kNoMatch) continue;
                bids[b] = std::max(bids[b], match_key(match_bits(values[(size_t)i * stride + r]), (uint32_t)a));
            }
        }
    uint32_t added = 0;
    if (flags & kMatchAccept)
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t a = (uint64_t)first + i;
            if (a >= n_a || match_a[a] != kNoMatch) continue;
            const uint64_t best = match_row_best(counts, keys, values, i, stride, n_b, match_b);
            if (!best) continue;
            const uint32_t b = match_key_end(best);
            if (bids[b] != ((best & 0xFFFFFFFF00000000ull) | (0xFFFFFFFFu - (uint32_t)a))) continue;
            match_a[a] = b;
            match_b[b] = (uint32_t)a;
            ++added;
        }
    return added;
}

#if defined(__HIPCC__)
// ngsMatchDevice: the steps `flags` names, in the order INIT, BEGIN, BID, ACCEPT, queued on s;
// nothing waits. matched: one word, the pairs so far (ACCEPT adds to it).
hipError_t launch_match(const uint32_t* counts, const uint32_t* keys, const float* values, uint32_t n, uint32_t stride,
                        uint32_t first, uint32_t* match_a, uint32_t n_a, uint32_t* match_b, uint32_t n_b,
                        uint64_t* bids, uint32_t* matched, uint32_t flags, hipStream_t s);
// NGS_LINK_BEST over one block: match_a[first + i] = the b of row i's first edge (b < n_b), kNoMatch
// for a row without one; *matched grows by the rows that got one.
hipError_t launch_match_best(const uint32_t* counts, const uint32_t* keys, const float* values, uint32_t n,
                             uint32_t stride, uint32_t first, uint32_t* match_a, uint32_t n_a, uint32_t n_b,
                             uint32_t* matched, hipStream_t s);
// The chosen record of every row: out_scores[first + i] / out_sims[first + i] = the score and the
// similarity of row i's record of key match_a[first + i] (the one of the largest value, the first
// among equals); 0.0f / -1.0f for an unmatched row. sims null: out_sims is -1.0f everywhere.
hipError_t launch_match_gather(const uint32_t* counts, const uint32_t* keys, const float* scores, const float* sims,
                               uint32_t n, uint32_t stride, uint32_t first, const uint32_t* match_a, uint32_t n_a,
                               float* out_scores, float* out_sims, hipStream_t s);
#endif

}  // namespace ngs
