// ngs_match.hip — the greedy one-to-one matching of a candidate block in rounds,
// for gfx950.
//
// k_match_bid     a group of lanes per row: every live edge raises bids[b] with one 64-bit atomic max
//                 that returns nothing;
// k_match_rows    a group of lanes per row: the row's largest live edge by shuffles, taken when
//                 bids[] names that very edge (kBest: the row's largest edge, taken as it is); the
//                 pairs counted with one atomic per wave;
// k_match_gather  the score and the similarity of every row's chosen record.
// The rows use k_union's shape: g = 2^lg lanes per row (the stride rounded up to a power of two, 64
// at the most), a lane taking the records r = its place in the group, + g, ...
#include <hip/hip_runtime.h>

#include "ngs_common.h"
#include "ngs_match.h"

namespace ngs {
namespace {

// match_b[] cells are written by other waves while k_match_rows reads them: relaxed agent-scope
// atomics. A row may see another row's match of the same round or miss it, and both are right
// (ngs_match.h): a cell only ever goes from kNoMatch to the end of an edge the sequential pass takes.
__device__ __forceinline__ uint32_t ld_match(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_match(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the largest key of the g lanes of a group, in every one of them (every lane of the wave calls it)
__device__ __forceinline__ uint64_t group_max(uint64_t v, uint32_t lg) {
    for (uint32_t o = (1u << lg) >> 1; o; o >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)o, 64);
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)o, 64);
        const uint64_t w = ((uint64_t)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// No match array is written in this launch: plain loads.
__global__ __launch_bounds__(256) void k_match_bid(const uint32_t* __restrict__ counts,
                                                   const uint32_t* __restrict__ keys,
                                                   const float* __restrict__ values, uint32_t n, uint32_t stride,
                                                   uint32_t first, const uint32_t* __restrict__ match_a, uint32_t n_a,
                                                   const uint32_t* __restrict__ match_b, uint32_t n_b,
                                                   unsigned long long* bids, uint32_t lg) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = t >> lg;
    if (row >= n) return;
    const uint64_t a = (uint64_t)first + row;
    if (a >= n_a || match_a[a] != kNoMatch) return;  // a matched row costs this one word
    const uint32_t count = min(counts[row], stride);
    const uint32_t* k = keys + row * stride;
    const float* v = values + row * stride;
    for (uint32_t r = (uint32_t)t & ((1u << lg) - 1u); r < count; r += 1u << lg) {
        const uint32_t b = k[r];
        if (b >= n_b || match_b[b] != kNoMatch) continue;  // nothing is read through an id past the arrays
        (void)atomicMax(bids + b, (unsigned long long)match_key(__float_as_uint(v[r]), (uint32_t)a));
    }
}

template <bool kBest>
__global__ __launch_bounds__(256) void k_match_rows(const uint32_t* __restrict__ counts,
                                                    const uint32_t* __restrict__ keys,
                                                    const float* __restrict__ values, uint32_t n, uint32_t stride,
                                                    uint32_t first, uint32_t* match_a, uint32_t n_a, uint32_t* match_b,
                                                    uint32_t n_b, const unsigned long long* __restrict__ bids,
                                                    uint32_t* matched, uint32_t lg) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = t >> lg;
    const uint64_t a = (uint64_t)first + row;
    // the lanes of a group agree on all of this: only its own row writes match_a[a]
    const bool open = row < n && a < n_a && (kBest || match_a[a] == kNoMatch);
    uint64_t best = 0;
    if (open) {
        const uint32_t count = min(counts[row], stride);
        const uint32_t* k = keys + row * stride;
        const float* v = values + row * stride;
        for (uint32_t r = (uint32_t)t & ((1u << lg) - 1u); r < count; r += 1u << lg) {
            const uint32_t b = k[r];
            if (b >= n_b) continue;
            if (!kBest && ld_match(match_b + b) != kNoMatch) continue;
            const uint64_t key = match_key(__float_as_uint(v[r]), b);
            best = key > best ? key : best;
        }
    }
    best = group_max(best, lg);
    bool won = false;
    if (open && ((uint32_t)t & ((1u << lg) - 1u)) == 0) {
        if (kBest) {
            match_a[a] = best ? match_key_end(best) : kNoMatch;
            won = best != 0;
        } else if (best) {
            const uint32_t b = match_key_end(best);
            // the same value, seen from b: the edge is the largest at both ends
            if (bids[b] == ((best & 0xFFFFFFFF00000000ull) | (0xFFFFFFFFu - (uint32_t)a))) {
                match_a[a] = b;
                st_match(match_b + b, (uint32_t)a);
                won = true;
            }
        }
    }
    const uint64_t wins = __ballot(won);
    if (wins && (threadIdx.x & 63u) == (uint32_t)__ffsll((unsigned long long)wins) - 1u)
        (void)atomicAdd(matched, (uint32_t)__popcll(wins));
}

__global__ __launch_bounds__(256) void k_match_gather(const uint32_t* __restrict__ counts,
                                                      const uint32_t* __restrict__ keys,
                                                      const float* __restrict__ scores, const float* __restrict__ sims,
                                                      uint32_t n, uint32_t stride, uint32_t first,
                                                      const uint32_t* __restrict__ match_a, uint32_t n_a,
                                                      float* __restrict__ out_scores, float* __restrict__ out_sims,
                                                      uint32_t lg) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = t >> lg;
    const uint64_t a = (uint64_t)first + row;
    const bool open = row < n && a < n_a;
    const uint32_t b = open ? match_a[a] : kNoMatch;
    const float* v = sims ? sims : scores;
    // the chosen record as (value, 0xFFFFFFFF - r): the largest value, the first among equals
    uint64_t best = 0;
    if (b != kNoMatch) {
        const uint32_t count = min(counts[row], stride);
        for (uint32_t r = (uint32_t)t & ((1u << lg) - 1u); r < count; r += 1u << lg) {
            if (keys[row * stride + r] != b) continue;
            const uint64_t key = match_key(__float_as_uint(v[row * stride + r]), r);
            best = key > best ? key : best;
        }
    }
    best = group_max(best, lg);
    if (open && ((uint32_t)t & ((1u << lg) - 1u)) == 0) {
        const uint64_t at = row * stride + match_key_end(best);  // (read only when best != 0)
        out_scores[a] = best ? scores[at] : 0.0f;
        out_sims[a] = best && sims ? sims[at] : kSimNone;
    }
}

// lanes per row (as a shift) and the blocks of n rows; false: too many blocks
bool row_grid(uint32_t n, uint32_t stride, uint32_t& lg, uint32_t& blocks) {
    lg = 0;
    while (lg < 6u && (1u << lg) < stride) ++lg;
    const uint64_t b = (((uint64_t)n << lg) + 255u) / 256u;
    blocks = (uint32_t)b;
    return b <= 0x7FFFFFFFull;
}

}  // namespace

hipError_t launch_match(const uint32_t* counts, const uint32_t* keys, const float* values, uint32_t n, uint32_t stride,
                        uint32_t first, uint32_t* match_a, uint32_t n_a, uint32_t* match_b, uint32_t n_b,
                        uint64_t* bids, uint32_t* matched, uint32_t flags, hipStream_t s) {
    if (flags & kMatchInit) {
        if (n_a)
            if (hipError_t e = hipMemsetAsync(match_a, 0xFF, sizeof(uint32_t) * (size_t)n_a, s); e != hipSuccess) return e;
        if (n_b)
            if (hipError_t e = hipMemsetAsync(match_b, 0xFF, sizeof(uint32_t) * (size_t)n_b, s); e != hipSuccess) return e;
        if (hipError_t e = hipMemsetAsync(matched, 0, sizeof(uint32_t), s); e != hipSuccess) return e;
    }
    if ((flags & kMatchBegin) && n_b)
        if (hipError_t e = hipMemsetAsync(bids, 0, sizeof(uint64_t) * (size_t)n_b, s); e != hipSuccess) return e;
    if (!n || !stride || !n_a || !n_b) return hipSuccess;  // no edge
    uint32_t lg = 0, blocks = 0;
    if (!row_grid(n, stride, lg, blocks)) return hipErrorInvalidValue;
    if (flags & kMatchBid) {
        hipLaunchKernelGGL(k_match_bid, dim3(blocks), dim3(256), 0, s, counts, keys, values, n, stride, first, match_a,
                           n_a, match_b, n_b, reinterpret_cast<unsigned long long*>(bids), lg);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (flags & kMatchAccept) {
        hipLaunchKernelGGL(k_match_rows<false>, dim3(blocks), dim3(256), 0, s, counts, keys, values, n, stride, first,
                           match_a, n_a, match_b, n_b, reinterpret_cast<const unsigned long long*>(bids), matched, lg);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_match_best(const uint32_t* counts, const uint32_t* keys, const float* values, uint32_t n,
                             uint32_t stride, uint32_t first, uint32_t* match_a, uint32_t n_a, uint32_t n_b,
                             uint32_t* matched, hipStream_t s) {
    if (!n) return hipSuccess;
    uint32_t lg = 0, blocks = 0;
    if (!row_grid(n, stride, lg, blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_match_rows<true>, dim3(blocks), dim3(256), 0, s, counts, keys, values, n, stride, first,
                       match_a, n_a, nullptr, n_b, nullptr, matched, lg);
    return hipGetLastError();
}

hipError_t launch_match_gather(const uint32_t* counts, const uint32_t* keys, const float* scores, const float* sims,
                               uint32_t n, uint32_t stride, uint32_t first, const uint32_t* match_a, uint32_t n_a,
                               float* out_scores, float* out_sims, hipStream_t s) {
    if (!n) return hipSuccess;
    uint32_t lg = 0, blocks = 0;
    if (!row_grid(n, stride, lg, blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_match_gather, dim3(blocks), dim3(256), 0, s, counts, keys, scores, sims, n, stride, first,
                       match_a, n_a, out_scores, out_sims, lg);
    return hipGetLastError();
}

}  // namespace ngs
