// ngs_set.h — index sets: the result blocks of several indexes for the same queries
// merged into the block one index over all their rows would have given. The definitions shared by
// the host reference routine and the device kernels (ngs_set.hip).
//
// A part p (0 <= p < P <= kSetMaxParts) is a result block in ngsSearchDevice's layout for the same n
// queries: counts_p[n], the records of row i at i * stride_p (a count above the stride is read as the
// stride), a key base base_p and a key-length table len_p[nKeys_p] (characters of the key as ngsKey /
// ngsKeyW returns it, without the NUL). A record is (p, k, s): part, local key id, fp32 score.
//
// Merge order. Records are totally ordered by
//   1. sim_order_bits(bits(s)) descending (ngs_sim.h: numeric order for non-NaN floats with -0 < +0,
//      a NaN where its bits put it),
//   2. len_p[k] ascending, 0xFFFFFFFF for k >= nKeys_p (nothing is read through such an id),
//   3. p ascending,
//   4. k ascending.
// Row i of the output is the first min(L, sum_p min(counts_p[i], stride_p)) records of the union in
// that order, L = limit ? limit : 2^31-1, each written as key base_p + k (u32 arithmetic) with its
// score bits unchanged; counts[i] is that number, cells past it are unspecified and nothing at or
// beyond i * out_stride + out_stride is written.
//
// Why this is the whole library's answer: a key's score depends on its own row only, a result row is
// (score descending, key id ascending), and key ids are ranks by (length ascending, first appearance
// ascending). For a library cut into contiguous row ranges with no master key in two of them the
// whole library's order is therefore (score desc, length asc, part asc, local id asc), and the top L
// of the union lies in the union of the parts' top L.
//
// Duplicate keys. Parts are not interned against each other: a master key that is present in two
// parts gives two records, under two global ids.
//
// Precondition the kernel uses: within a part a row is already in merge order (ngsSearchDevice's rows
// are: score descending, then k ascending, and k ascends with the length). For a row that is not,
// the order of the output is unspecified; counts[i] is still the number above, every access stays in
// bounds and every written record is one of the inputs.
//
// Plain C++17 without a HIP include: g++ compiles the host routine alone (tests/sanitize).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ngs_sim.h"

namespace ngs {

constexpr uint32_t kSetMaxParts = 16;            // NGS_SET_MAX_PARTS
constexpr uint32_t kSetNoLen = 0xFFFFFFFFu;      // the length of a key id past its part's table
constexpr uint32_t kSetLimitAll = 0x7FFFFFFFu;   // limit 0
// k_merge_parts' cut-overs (the tests sit on them):
//  - a launch whose rows hold at most kSetOneWaveRecords records each (sum_p min(stride_p, L)) runs
//    one wave per query, any other a workgroup of kSetThreads;
//  - a query whose rows hold at most kSetLdsRecords records (sum_p min(counts_p[i], stride_p, L))
//    stages their comparators in LDS (8 bytes each: 64,000 bytes, which with the row's bookkeeping
//    stays within the 64 KiB a launch gets without asking for more), any other reads them from HBM.
constexpr uint32_t kSetOneWaveRecords = 256;
constexpr uint32_t kSetThreads = 256;
constexpr uint32_t kSetLdsRecords = 8000;

// One part as the kernel takes it, by value: 16 of them are the 768 bytes of MergeParts.
struct MergePart {
    const uint32_t* counts;
    const uint32_t* keys;
    const float* scores;
    const uint32_t* len;
    uint32_t stride, base, n_keys, pad;
};
static_assert(sizeof(MergePart) == 48, "16 parts x 48 bytes travel in the kernel arguments");
struct MergeParts {
    MergePart p[kSetMaxParts];
};

// The comparator of a record: smaller = earlier. Ties are settled by (p, k).
NGS_HD inline uint64_t set_cmp(uint32_t score_bits, uint32_t len) {
    return ((uint64_t)(~sim_order_bits(score_bits)) << 32) | len;
}
NGS_HD inline uint32_t set_limit(uint32_t limit) { return limit ? limit : kSetLimitAll; }

// ---- host reference routine (the kernel restates it as a merge by ranks) ----
// Row i of the merge of P parts into out_keys / out_scores at i * out_stride: a plain stable sort of
// the union. Returns the row's count. The caller's out_stride is at least min(L, sum_p stride_p).
inline uint32_t merge_row(const MergePart* parts, uint32_t P, uint32_t i, uint32_t limit, uint32_t out_stride,
                          uint32_t* out_keys, float* out_scores) {
    struct Rec {
        uint64_t cmp;
        uint32_t p, k, bits;
    };
    std::vector<Rec> recs;
    for (uint32_t p = 0; p < P; ++p) {
        const MergePart& M = parts[p];
        const uint32_t c = M.counts[i] < M.stride ? M.counts[i] : M.stride;
        for (uint32_t r = 0; r < c; ++r) {
            const uint32_t k = M.keys[(size_t)i * M.stride + r];
            uint32_t bits;
            std::memcpy(&bits, M.scores + (size_t)i * M.stride + r, sizeof bits);
            recs.push_back({set_cmp(bits, k < M.n_keys ? M.len[k] : kSetNoLen), p, k, bits});
        }
    }
    std::stable_sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) {
        if (a.cmp != b.cmp) return a.cmp < b.cmp;
        if (a.p != b.p) return a.p < b.p;
        return a.k < b.k;
    });
    const uint64_t L = set_limit(limit);
    const uint32_t n = (uint32_t)(recs.size() < L ? recs.size() : L);
    for (uint32_t r = 0; r < n; ++r) {
        out_keys[(size_t)i * out_stride + r] = parts[recs[r].p].base + recs[r].k;
        std::memcpy(out_scores + (size_t)i * out_stride + r, &recs[r].bits, sizeof(float));
    }
    return n;
}
inline void merge_rows(const MergePart* parts, uint32_t P, uint32_t n, uint32_t limit, uint32_t out_stride,
                       uint32_t* out_counts, uint32_t* out_keys, float* out_scores) {
    for (uint32_t i = 0; i < n; ++i) out_counts[i] = merge_row(parts, P, i, limit, out_stride, out_keys, out_scores);
}
// the least out_stride a merge may be given: min(L, sum_p stride_p), the sum in 64 bits
inline uint64_t merge_min_stride(const MergePart* parts, uint32_t P, uint32_t limit) {
    uint64_t sum = 0;
    for (uint32_t p = 0; p < P; ++p) sum += parts[p].stride;
    return std::min<uint64_t>(sum, set_limit(limit));
}

// ---- the similarity over a set ----
// A record is (query i, global key id g). Member p owns g iff base_p <= g < base_p + nKeys_p; the
// members tile [0, total) in order (base_0 = 0, base_{p+1} = base_p + nKeys_p; a member may be empty).
// The record's similarity and matched term are those of ngsSimilarityDeviceM for the local key
// g - base_p on member p (ngs_sim.h: metric, wildcard rule, kSimMaxQuery, the fp32 formula); the term
// id is the member's local one. g >= total gives kSimNone and kSimNoTerm, nothing read through it.
// The query is normalised once, with the validChar set of the set's first member: a caller who
// changes one member's set changes them all (§9.7).
//
// The members as k_sim_set takes them, by value (ngs_sim.h: SimMember); members of both storage
// forms mix in one launch.
struct SimMembers {
    SimMember m[kSetMaxParts];
};
constexpr uint32_t kSetNoPart = 0xFFFFFFFFu;  // no member owns the id

// ---- host reference routines (k_sim_set restates them per lane) ----
// The member owning g among P members of ascending bases: the last whose base is at or below g
// (empty members share a base with their successor and own nothing); kSetNoPart for g >= total.
inline uint32_t sim_set_part(const SimMember* m, uint32_t P, uint32_t g) {
    if (P == 0 || (uint64_t)g >= (uint64_t)m[P - 1].base + m[P - 1].n_keys) return kSetNoPart;
    uint32_t p = 0;
    for (uint32_t i = 1; i < P; ++i) p += m[i].base <= g ? 1u : 0u;
    return p;
}
// The record rule: the member p and the local key of g, and the member's local term ids the record
// compares, in order, into terms[0 .. returned count) (at most cap are written). A term id at or
// past n_terms is skipped as the kernel skips it. False, and nothing read through g, for g >= total.
inline bool sim_set_record(const SimMember* m, uint32_t P, uint32_t g, uint32_t& p, uint32_t& key, uint32_t* terms,
                           uint32_t cap, uint32_t& n_terms) {
    n_terms = 0;
    p = sim_set_part(m, P, g);
    if (p == kSetNoPart) return false;
    const SimMember& M = m[p];
    key = g - M.base;
    const uint32_t j = M.kt_off ? M.kt_off[key] : 0u, je = M.kt_off ? M.kt_off[key + 1] : 1u;
    for (uint32_t i = j; i < je; ++i) {
        const uint32_t t = M.kt_off ? M.kt_term[i] : M.key_term[key];
        if (t >= M.n_terms) continue;
        if (n_terms < cap) terms[n_terms] = t;
        ++n_terms;
    }
    return true;
}

// ---- dead keys: delete without a rebuild ----
// Definition. A set keeps, per member, a dead mask of one bit per local key id (bit k & 31 of word
// k >> 5). Every answer of a set with dead keys is the answer of a set over the same members with the
// rows of the dead master keys left out, compared by key string, order and fp32 score bits; the
// global key ids are the unchanged ones of the full set (base_p + k), so ids are stable under delete
// as they are under append. The members themselves are never changed.
//
// Why it is exact: a key's score depends on its own row only, and the whole library's order is
// (score desc, length asc, part asc, local id asc). Removing records from a totally ordered list
// keeps the order of the rest.
//
// Row rule (drop_dead_row, k_drop_dead). Row i of a block in ngsSearchDevice's layout, in place: with
// c = min(counts[i], stride), every record whose key k < n_keys has its dead bit set is removed (a
// k >= n_keys is live, nothing is read through it); the remaining records keep their order and move
// up; the row is cut to L = limit ? limit : 2^31-1; counts[i] is the new count. Cells past the new
// count are unspecified, nothing at or beyond i * stride + stride is written. A row is short when
// c == stride and fewer than L records are left: the search may have had more hits behind the block.
//
// The over-fetch (set_search). A member with d dead keys is searched at limit L + E into a block of
// stride min(L + E, n_keys), then cut to L by the rule above. With E = d that is exact: the top L + d
// of all keys hold the top L of the live ones. E starts at dead_first_fetch: what fills the search's
// one-wave tier, kSetDeadFastLimit - L, while that is at least kSetDeadFetchMin (a search at a limit
// above kSetDeadFastLimit leaves that tier for every query; §9.9 has what the two choices measured),
// else max(L, kSetDeadFetch0); never more than d. A
// member with a short row whose stride was below both L + d and n_keys is searched again with E grown
// by kSetDeadFetchGrowth, capped at d (dead_next_fetch), until none is left.
constexpr uint32_t kSetDeadFetch0 = 64;
constexpr uint32_t kSetDeadFetchGrowth = 4;
constexpr uint32_t kSetDeadFastLimit = 128;  // kWaveMaxLimit (ngs_common.h; ngs_abi.cpp asserts it)
constexpr uint32_t kSetDeadFetchMin = 16;

NGS_HD inline bool dead_bit(const uint32_t* dead, uint32_t n_keys, uint32_t k) {
    return k < n_keys && ((dead[k >> 5] >> (k & 31u)) & 1u) != 0u;
}
// the first over-fetch of a member with d dead keys at limit L (= set_limit(limit))
inline uint32_t dead_first_fetch(uint32_t d, uint32_t L) {
    const bool fast = L <= kSetDeadFastLimit - kSetDeadFetchMin;
    return std::min(d, fast ? kSetDeadFastLimit - L : std::max(L, kSetDeadFetch0));
}
// the one after E (0 < E < d)
inline uint32_t dead_next_fetch(uint32_t d, uint32_t E) {
    return (uint32_t)std::min<uint64_t>(d, (uint64_t)E * kSetDeadFetchGrowth);
}
// the stride of a member of n_keys keys searched at L + E: min(L + E, n_keys), the sum in 64 bits
// (at or above 2^31-1 it means "all")
inline uint32_t dead_fetch_stride(uint32_t L, uint32_t E, uint32_t n_keys) {
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>((uint64_t)L + E, kSetLimitAll), n_keys);
}

// One block as k_drop_dead takes it, by value: 16 of them are the 768 bytes of DropBlocks.
struct DropBlock {
    uint32_t* counts;
    uint32_t* keys;
    float* scores;
    const uint32_t* dead;
    uint32_t* n_short;  // += the block's short rows (may be null)
    uint32_t stride, n_keys;
};
static_assert(sizeof(DropBlock) == 48, "16 blocks x 48 bytes travel in the kernel arguments");
struct DropBlocks {
    DropBlock b[kSetMaxParts];
};

// ---- host reference routine (k_drop_dead restates it as a compaction by ballots) ----
// The row rule on one row (keys / scores point at its first cell): returns the new count, and whether
// the row is short in *is_short (may be null).
inline uint32_t drop_dead_row(uint32_t count, uint32_t stride, uint32_t* keys, float* scores, const uint32_t* dead,
                              uint32_t n_keys, uint32_t limit, bool* is_short) {
    const uint32_t c = count < stride ? count : stride;
    const uint32_t L = set_limit(limit);
    uint32_t live = 0;
    for (uint32_t r = 0; r < c; ++r) {
        if (dead_bit(dead, n_keys, keys[r])) continue;
        if (live < L && live != r) {
            keys[live] = keys[r];
            std::memcpy(scores + live, scores + r, sizeof(float));
        }
        ++live;
    }
    if (is_short) *is_short = c == stride && live < L;
    return live < L ? live : L;
}

#if defined(__HIPCC__)
// k_drop_dead over nb blocks of n rows each, in one launch (a grid over (row, block)); queued on s,
// waits for nothing
hipError_t launch_drop_dead(const DropBlocks& blocks, uint32_t nb, uint32_t n, uint32_t limit, hipStream_t s);
// counts[i] = 0 for every row i < n whose global key id first + i is dead in its member (P members of
// ascending bases, as SimMembers'; dead[p] may be null: no dead key there)
struct DeadMasks {
    const uint32_t* dead[kSetMaxParts];
    uint32_t base[kSetMaxParts], n_keys[kSetMaxParts];
};
hipError_t launch_zero_dead_rows(const DeadMasks& masks, uint32_t P, uint32_t* counts, uint32_t n, uint32_t first,
                                 hipStream_t s);
// launch_similarity over the P members of T (character size cs, the first member's validChar set):
// one launch for the whole block; terms (may be null) receives the members' local term ids.
hipError_t launch_similarity_set(const SimMembers& T, uint32_t P, uint32_t cs, const uint32_t valid[8],
                                 const uint8_t* raw, const uint64_t* off, uint32_t n, uint32_t stride,
                                 const uint32_t* counts, const uint32_t* keys, uint32_t metric, float* sim,
                                 uint32_t* terms, hipStream_t s);
// Both queue on s and wait for nothing.
// len[i] = characters of key first + i (key_off counts characters, one NUL per key)
hipError_t launch_key_len(const uint64_t* key_off, uint32_t first, uint32_t n, uint32_t* len, hipStream_t s);
hipError_t launch_merge_parts(const MergeParts& parts, uint32_t P, uint32_t n, uint32_t limit, uint32_t out_stride,
                              uint32_t* out_counts, uint32_t* out_keys, float* out_scores, hipStream_t s);
#endif

}  // namespace ngs
