// ngs_join.h — the self-join of the library and the clusters of its keys: the
// definitions shared by the host routines and the device kernels (ngs_join.hip).
//
// The join of keys [first, first + n): row i is the search's answer for the raw string of key
// first + i without that key's own record. Three stages stand around ngsSearchDevice:
//   gather     the keys as a query batch, straight from DevIndex.key_off / key_bytes;
//   drop-self  the record (first + i) of row i removed, the gap closed, the row cut to the limit;
//   cluster    a union-find over the (key, key) records: labels[k] = smallest id of k's component.
//
// Plain C++17 without a HIP include: g++ compiles the host routines alone (tests/sanitize).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "ngs_common.h"
#endif
#ifndef NGS_HD
#if defined(__HIPCC__)
#define NGS_HD __host__ __device__
#else
#define NGS_HD
#endif
#endif

namespace ngs {

constexpr uint32_t kJoinBatchKeys = 65536;  // keys per batch of selfJoin / dedupKeys (bench C3's batch)
constexpr uint32_t kClusterInit = 1u;       // NGS_CLUSTER_INIT
constexpr uint32_t kClusterFinish = 2u;     // NGS_CLUSTER_FINISH

// key_off counts one NUL per key, so the characters of the keys [first, first + i) without their
// NULs are key_off[first + i] - key_off[first] - i: query i of the batch starts there (no scan).
NGS_HD inline uint64_t join_query_off(const uint64_t* key_off, uint32_t first, uint32_t i, uint32_t cs) {
    return (key_off[first + i] - key_off[first] - i) * cs;
}

// the records a row keeps: `count` of them (read as at most the stride), one less when its own
// record is among them, cut to `limit` (0: no cut)
NGS_HD inline uint32_t join_row_count(uint32_t count, bool has_self, uint32_t limit) {
    const uint32_t c = has_self ? count - 1u : count;
    return limit && c > limit ? limit : c;
}

// ---- host reference routines (the kernels restate them per wave / with atomics) ----
// One row in place: the record whose key is `self` removed (at most one exists), the later records
// moved up by one, the row cut to `limit`. Returns the new count; cells past it keep what they held.
inline uint32_t drop_self_row(uint32_t* keys, float* scores, uint32_t count, uint32_t stride, uint64_t self,
                              uint32_t limit) {
    if (count > stride) count = stride;
    uint32_t p = count;
    for (uint32_t r = 0; r < count; ++r)
        if (keys[r] == self) {
            p = r;
            break;
        }
    const uint32_t kept = join_row_count(count, p < count, limit);
    for (uint32_t r = p; r < kept; ++r) {
        keys[r] = keys[r + 1];
        scores[r] = scores[r + 1];
    }
    return kept;
}

// Union-find over parent[] with parent[x] <= x: find with path halving, the root with the larger
// id hooked under the smaller one. The root of a tree is the smallest id of its component.
inline uint32_t uf_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = parent[x];
        if (p == x) return x;
        const uint32_t gp = parent[p];
        parent[x] = gp;
        x = gp;
    }
}
inline void uf_union(uint32_t* parent, uint32_t a, uint32_t b) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) parent[b] = a;
    else parent[a] = b;
}
// the block's edges (first + i, keys[i * stride + r]) merged into parent[n_labels]; an edge with an
// end >= n_labels is ignored
inline void uf_block(uint32_t* parent, uint32_t n_labels, const uint32_t* counts, const uint32_t* keys, uint32_t n,
                     uint32_t stride, uint32_t first) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t a = (uint64_t)first + i;
        const uint32_t c = counts[i] < stride ? counts[i] : stride;
        for (uint32_t r = 0; r < c; ++r) {
            const uint32_t b = keys[(size_t)i * stride + r];
            if (a < n_labels && b < n_labels) uf_union(parent, (uint32_t)a, b);
        }
    }
}
inline void uf_finish(uint32_t* parent, uint32_t n_labels) {
    for (uint32_t k = 0; k < n_labels; ++k) parent[k] = uf_find(parent, k);
}

#if defined(__HIPCC__)
// Everything below queues on s and waits for nothing.
// off[0..n] and the bytes of keys [first, first + n) as a query batch; total = join_query_off(.., n, ..)
hipError_t launch_key_queries(const DevIndex& X, uint32_t first, uint32_t n, uint64_t total, uint8_t* bytes,
                              uint64_t* off, hipStream_t s);
// off[i] += add, i < n: the offsets of a batch gathered behind another one's bytes
hipError_t launch_shift_offsets(uint64_t* off, uint64_t n, uint64_t add, hipStream_t s);
hipError_t launch_drop_self(uint32_t* counts, uint32_t* keys, float* scores, uint32_t n, uint32_t stride,
                            uint32_t first, uint32_t limit, hipStream_t s);
// records with sim < min_sim removed from every row, the others kept in order (keys and scores; with
// sim_out = sim their similarities too, so that sim stays in the records' layout)
hipError_t launch_keep_similar(uint32_t* counts, uint32_t* keys, float* scores, const float* sim, uint32_t n,
                               uint32_t stride, float min_sim, hipStream_t s, float* sim_out = nullptr);
hipError_t launch_cluster(const uint32_t* counts, const uint32_t* keys, uint32_t n, uint32_t stride, uint32_t first,
                          uint32_t* labels, uint32_t n_labels, uint32_t flags, hipStream_t s);
#endif

}  // namespace ngs
