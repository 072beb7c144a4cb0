// ngs_set.hip — index sets, for gfx950.
//
// k_key_len      len[i] = the characters of key first + i, from two neighbouring key_off cells;
// k_merge_parts  one workgroup per query: the P sorted rows merged by ranks. The output position of
//                record r of part p is r plus, for every other part, the number of that part's
//                records that precede it: a binary search over that part's row (an upper bound in
//                the parts before p, a lower bound in those behind it, which is the (p, k) tie
//                rule). No sort, no atomics: a record's place depends on the inputs alone.
// The comparators ((~order bits << 32) | length, ngs_set.h) of a query whose rows hold at most
// kSetLdsRecords records are staged in dynamic LDS, part after part; a larger query takes the same
// ranks with every probe's comparator read from HBM (score, key id, then the key's length).
#include <hip/hip_runtime.h>

#include "ngs_common.h"
#include "ngs_set.h"

namespace ngs {
namespace {

__global__ __launch_bounds__(256) void k_key_len(const uint64_t* __restrict__ key_off, uint32_t first, uint32_t n,
                                                 uint32_t* __restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) len[i] = (uint32_t)(key_off[first + i + 1] - key_off[first + i] - 1u);
}

// record r of row `row` of part M: its comparator from HBM (the one scattered read is M.len[k])
__device__ __forceinline__ uint64_t cmp_hbm(const MergePart& M, uint64_t row, uint32_t r) {
    const uint64_t at = row * M.stride + r;
    const uint32_t k = M.keys[at];
    return set_cmp(__float_as_uint(M.scores[at]), k < M.n_keys ? M.len[k] : kSetNoLen);
}

// the records among the c sorted ones that precede a record of comparator x: those < x, and with
// `ties` those == x too. get(j) is the comparator of record j.
template <class Get>
__device__ __forceinline__ uint32_t preceding(uint32_t c, uint64_t x, bool ties, Get get) {
    uint32_t lo = 0, hi = c;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = get(mid);
        if (v < x || (ties && v == x)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kSetThreads) void k_merge_parts(const MergeParts A, uint32_t P, uint32_t limit,
                                                            uint32_t out_stride, uint32_t lds_records,
                                                            uint32_t* __restrict__ out_counts,
                                                            uint32_t* __restrict__ out_keys,
                                                            float* __restrict__ out_scores) {
    extern __shared__ uint64_t s_cmp[];
    // the records of each part that can reach the output and their starts in the staged order
    __shared__ uint32_t s_cnt[kSetMaxParts];
    __shared__ uint64_t s_start[kSetMaxParts + 1];
    const uint64_t row = blockIdx.x;
    const uint32_t L = set_limit(limit);
    if (threadIdx.x < kSetMaxParts) {
        const uint32_t p = threadIdx.x;
        s_cnt[p] = p < P ? min(A.p[p].counts[row], A.p[p].stride) : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = 0, at = 0;
        for (uint32_t p = 0; p < kSetMaxParts; ++p) {
            const uint32_t c = s_cnt[p];
            all += c;
            s_cnt[p] = min(c, L);
            s_start[p] = at;
            at += min(c, L);
        }
        s_start[kSetMaxParts] = at;
        out_counts[row] = (uint32_t)(all < L ? all : L);
    }
    __syncthreads();
    const uint64_t total = s_start[kSetMaxParts];
    const bool staged = total <= lds_records;  // uniform over the workgroup
    // the part of staged record t (parts past P start at `total`: the answer is < P)
    auto part_of = [&](uint64_t t) {
        uint32_t p = 0;
        for (uint32_t q = 1; q < P; ++q) p += t >= s_start[q] ? 1u : 0u;
        return p;
    };
    if (staged) {
        for (uint32_t t = threadIdx.x; t < (uint32_t)total; t += blockDim.x) {
            const uint32_t p = part_of(t);
            s_cmp[t] = cmp_hbm(A.p[p], row, t - (uint32_t)s_start[p]);
        }
        __syncthreads();
    }
    for (uint64_t t = threadIdx.x; t < total; t += blockDim.x) {
        const uint32_t p = part_of(t);
        const uint32_t r = (uint32_t)(t - s_start[p]);
        const uint64_t x = staged ? s_cmp[t] : cmp_hbm(A.p[p], row, r);
        uint64_t rank = r;
        for (uint32_t q = 0; q < P; ++q) {
            const uint32_t c = s_cnt[q];
            if (q == p || c == 0) continue;
            if (staged) {
                const uint64_t* v = s_cmp + s_start[q];
                rank += preceding(c, x, q < p, [&](uint32_t j) { return v[j]; });
            } else {
                rank += preceding(c, x, q < p, [&](uint32_t j) { return cmp_hbm(A.p[q], row, j); });
            }
        }
        // rank < total, and the caller's stride holds min(L, total) records
        if (rank < L && rank < out_stride) {
            const uint64_t at = row * A.p[p].stride + r;
            out_keys[row * out_stride + rank] = A.p[p].base + A.p[p].keys[at];
            out_scores[row * out_stride + rank] = A.p[p].scores[at];
        }
    }
}

}  // namespace

hipError_t launch_key_len(const uint64_t* key_off, uint32_t first, uint32_t n, uint32_t* len, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_key_len, dim3((uint32_t)(((uint64_t)n + 255u) / 256u)), dim3(256), 0, s, key_off, first, n, len);
    return hipGetLastError();
}

hipError_t launch_merge_parts(const MergeParts& parts, uint32_t P, uint32_t n, uint32_t limit, uint32_t out_stride,
                              uint32_t* out_counts, uint32_t* out_keys, float* out_scores, hipStream_t s) {
    if (!n) return hipSuccess;
    if (P == 0 || P > kSetMaxParts || n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    // the most records a row stages: the workgroup's size and its LDS follow it
    uint64_t bound = 0;
    for (uint32_t p = 0; p < P; ++p) bound += std::min(parts.p[p].stride, set_limit(limit));
    const uint32_t threads = bound <= kSetOneWaveRecords ? 64u : kSetThreads;
    const uint32_t lds_records = (uint32_t)std::min<uint64_t>(bound, kSetLdsRecords);
    hipLaunchKernelGGL(k_merge_parts, dim3(n), dim3(threads), sizeof(uint64_t) * lds_records, s, parts, P, limit,
                       out_stride, lds_records, out_counts, out_keys, out_scores);
    return hipGetLastError();
}

}  // namespace ngs
