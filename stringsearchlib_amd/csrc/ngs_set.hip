// ngs_set.hip — index sets, for gfx950.
//
// k_key_len      len[i] = the characters of key first + i, from two neighbouring key_off cells;
// k_merge_parts  one workgroup per query: the P sorted rows merged by ranks. The output position of
//                record r of part p is r plus, for every other part, the number of that part's
//                records that precede it: a binary search over that part's row (an upper bound in
//                the parts before p, a lower bound in those behind it, which is the (p, k) tie
//                rule). No sort, no atomics: a record's place depends on the inputs alone.
// k_drop_dead    one workgroup per (row, block): the records of dead keys (§9.9) removed in place by
//                ballots and prefix counts, the row cut to the limit, the short rows counted;
// k_zero_dead_rows  the rows of a join whose own key is dead emptied.
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

// drop_dead_row on row blockIdx.x of block blockIdx.y: a stable stream compaction in chunks of
// blockDim.x records (one wave, or kSetThreads). A lane's destination in a chunk is the running base
// plus the live records of the earlier waves (LDS) plus those of the earlier lanes of its own (the
// ballot below the lane). A record's destination never lies behind its source, and a chunk is read
// completely (every wave's loads waited for, then the barrier) before any of it is written, so the
// row is compacted in place; the next chunk's cells lie behind everything written so far.
__global__ __launch_bounds__(kSetThreads) void k_drop_dead(const DropBlocks A, uint32_t limit) {
    __shared__ uint32_t s_live[kSetThreads / 64];
    const DropBlock& B = A.b[blockIdx.y];
    const uint64_t row = blockIdx.x;
    const uint32_t L = set_limit(limit);
    const uint32_t c = min(B.counts[row], B.stride);
    uint32_t* keys = B.keys + row * B.stride;
    float* scores = B.scores + row * B.stride;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    uint32_t base = 0;  // the live records of the chunks so far: uniform over the workgroup
    for (uint64_t at = 0; at < c && base < L; at += blockDim.x) {  // (64 bits: c may be within a chunk of 2^32)
        const uint64_t r = at + threadIdx.x;
        const bool have = r < c;
        const uint32_t k = have ? keys[r] : 0u;
        const float sc = have ? scores[r] : 0.0f;
        const bool live = have && !dead_bit(B.dead, B.n_keys, k);
        const uint64_t mask = __ballot(live);
        uint32_t before = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), all = (uint32_t)__popcll(mask);
        __builtin_amdgcn_s_waitcnt(0);  // this wave's part of the chunk is in registers
        if (waves > 1) {
            if (lane == 0) s_live[wave] = all;
            __syncthreads();
            all = 0;
            for (uint32_t w = 0; w < waves; ++w) {
                const uint32_t v = s_live[w];
                before += w < wave ? v : 0u;
                all += v;
            }
            __syncthreads();  // (s_live is rewritten by the next chunk)
        }
        const uint32_t to = base + before;  // <= r
        if (live && to < L) {
            keys[to] = k;
            scores[to] = sc;
        }
        base += all;
    }
    if (threadIdx.x == 0) {
        B.counts[row] = min(base, L);
        if (B.n_short && c == B.stride && base < L) atomicAdd(B.n_short, 1u);
    }
}

// the member owning global key g (ngs_set.h: sim_set_part) and its dead bit
__global__ __launch_bounds__(256) void k_zero_dead_rows(const DeadMasks D, uint32_t P, uint32_t* __restrict__ counts,
                                                        uint32_t n, uint32_t first) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = (uint64_t)first + i;
    uint32_t p = 0;
    for (uint32_t q = 1; q < P; ++q) p += D.base[q] <= g ? 1u : 0u;
    if (g < (uint64_t)D.base[p] + D.n_keys[p] && D.dead[p] && dead_bit(D.dead[p], D.n_keys[p], (uint32_t)(g - D.base[p])))
        counts[i] = 0u;
}

}  // namespace

hipError_t launch_drop_dead(const DropBlocks& blocks, uint32_t nb, uint32_t n, uint32_t limit, hipStream_t s) {
    if (!n || !nb) return hipSuccess;
    if (nb > kSetMaxParts || n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    uint32_t most = 0;  // the most records a row holds
    for (uint32_t b = 0; b < nb; ++b) most = std::max(most, blocks.b[b].stride);
    const uint32_t threads = most <= kSetOneWaveRecords ? 64u : kSetThreads;
    hipLaunchKernelGGL(k_drop_dead, dim3(n, nb), dim3(threads), 0, s, blocks, limit);
    return hipGetLastError();
}

hipError_t launch_zero_dead_rows(const DeadMasks& masks, uint32_t P, uint32_t* counts, uint32_t n, uint32_t first,
                                 hipStream_t s) {
    if (!n || !P) return hipSuccess;
    if (P > kSetMaxParts) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_zero_dead_rows, dim3((uint32_t)(((uint64_t)n + 255u) / 256u)), dim3(256), 0, s, masks, P, counts,
                       n, first);
    return hipGetLastError();
}

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
