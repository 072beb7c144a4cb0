// ngs_token.hip — the token sort in front of the similarity (the rules: ngs_token.h),
// for gfx950.
//
// k_token_sort: one wave per string. The wave finds the trim with ballot windows as k_sim does, loads
// the span (at most kSimMaxQuery characters) into LDS, marks token starts and ends by ballot into a
// (start, length) table, orders the table (up to 64 tokens: every lane counts the tokens in front of
// its own; more: a bitonic sort over the table, the start as the last key, which makes the order
// total and so the result the stable one), scans the sorted lengths into output positions, and
// writes every output character by a search of its position: one pass of coalesced vector stores,
// after the last read of the string (so the output may lie over the input).
// kStored: the index's terms (normalised already; offsets in characters; the output ends at L').
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>
#include <type_traits>

#include "ngs_common.h"
#include "ngs_token.h"

namespace ngs {
namespace {

struct TokenArgs {
    const uint8_t* raw;
    const uint64_t* off;      // [n + 1]: bytes; kStored: characters
    uint8_t* out;
    const uint64_t* out_off;  // kStored: where the sorted terms go (characters); else the strings' own
    uint64_t* len_out;        // kStored pass 1: only the lengths L' are written, here
    uint32_t n;
    ValidSet V;
};

constexpr uint32_t kTokPad = 0xFFFFFFFFu;  // sorts behind every token (a token is start | length << 16)

template <bool kStored>
__device__ __forceinline__ bool tok_keeps(const uint32_t* valid, uint32_t c, uint32_t cs) {
    if constexpr (kStored) return !sim_space(c);
    else return sim_keeps(valid, c, cs);
}
template <bool kStored>
__device__ __forceinline__ uint32_t tok_norm(const uint32_t* valid, uint32_t c, uint32_t cs) {
    if constexpr (kStored) return c;
    else return sim_norm(valid, c, cs);
}

// token a sorts in front of token b: by the normalised characters, a proper prefix first, then by start
template <bool kStored, class CharT>
__device__ __forceinline__ bool tok_less(const CharT* ch, const uint32_t* valid, uint32_t a, uint32_t b) {
    if (a == b || a == kTokPad) return false;
    if (b == kTokPad) return true;
    const uint32_t sa = a & 0xFFFFu, la = a >> 16, sb = b & 0xFFFFu, lb = b >> 16;
    const uint32_t k = min(la, lb);
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t ca = tok_norm<kStored>(valid, ch[sa + i], sizeof(CharT));
        const uint32_t cb = tok_norm<kStored>(valid, ch[sb + i], sizeof(CharT));
        if (ca != cb) return ca < cb;
    }
    return la != lb ? la < lb : sa < sb;
}

template <bool kWide, bool kStored>
__global__ __launch_bounds__(64) void k_token_sort(TokenArgs A) {
    using CharT = std::conditional_t<kWide, uint32_t, uint8_t>;
    constexpr uint32_t cs = sizeof(CharT);
    __shared__ CharT s_chars[kSimMaxQuery];
    __shared__ uint32_t s_tok[kTokenMaxCount];
    __shared__ uint16_t s_pos[kTokenMaxCount];  // where a sorted token starts in the output
    __shared__ uint32_t s_valid[8];
    const uint32_t lane = threadIdx.x, q = blockIdx.x;
    if (lane < 8) s_valid[lane] = A.V.w[lane];
    __syncthreads();  // (the workgroup is one wave: the barriers here order its LDS accesses only)

    const uint64_t unit = kStored ? cs : 1u;
    const uint64_t qa = A.off[q] * unit, qe = A.off[q + 1] * unit;
    const uint64_t n = qe > qa ? (qe - qa) / cs : 0;
    const CharT* in = reinterpret_cast<const CharT*>(A.raw + qa);
    CharT* out = nullptr;
    if (!A.len_out) out = reinterpret_cast<CharT*>(A.out + (kStored ? A.out_off[q] * cs : qa));

    // the trim: everything here is uniform over the wave
    uint64_t first = n, m64 = 0;
    for (uint64_t base = 0; base < n; base += 64) {
        const uint64_t i = base + lane;
        const uint64_t bal = __ballot(i < n && tok_keeps<kStored>(s_valid, in[i < n ? i : 0], cs));
        if (bal) {
            first = base + (uint32_t)__ffsll((unsigned long long)bal) - 1u;
            break;
        }
    }
    if (first < n) {
        uint64_t last = first;
        for (uint64_t base = 0; base < n; base += 64) {
            const uint64_t i = base + lane;
            const uint64_t bal = __ballot(i < n && tok_keeps<kStored>(s_valid, in[i < n ? n - 1 - i : 0], cs));
            if (bal) {
                last = n - 1 - (base + (uint32_t)__ffsll((unsigned long long)bal) - 1u);
                break;
            }
        }
        m64 = last - first + 1;
    }
    // unchanged: a span the similarity does not take, and the wildcard "*" (which is a wildcard by its
    // raw characters, whether or not the validChar set keeps '*')
    if (m64 > kSimMaxQuery || (!kStored && n == 1 && in[0] == (CharT)'*')) {
        if (A.len_out) {
            if (lane == 0) A.len_out[q] = n;
            return;
        }
        if (out != in) {
            for (uint64_t i = lane; i < n; i += 64) out[i] = in[i];
            if (!kStored && kWide && lane < ((qe - qa) & 3u)) A.out[qa + n * cs + lane] = A.raw[qa + n * cs + lane];
        }
        return;
    }
    const uint32_t m = (uint32_t)m64;
    for (uint32_t i = lane; i < m; i += 64) s_chars[i] = in[first + i];
    __syncthreads();  // the string's last read: from here on the output may be written over it

    // tokens: a start is a kept character behind a separator, an end the separator (or the span's end)
    // behind a kept one; the k-th end closes the k-th start
    uint32_t count = 0, ends = 0, kept = 0;
    uint64_t carry = 0;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base <= m; base += 64) {
        const uint32_t i = base + lane;
        const uint64_t K = __ballot(i < m && tok_keeps<kStored>(s_valid, s_chars[i < m ? i : 0], cs));
        const uint64_t prev = (K << 1) | carry;
        const uint64_t S = K & ~prev, E = ~K & prev;
        carry = K >> 63;
        if ((S >> lane) & 1ull) {
            const uint32_t k = count + (uint32_t)__popcll(S & below);
            if (k < kTokenMaxCount) s_tok[k] = i;
        }
        __syncthreads();
        if ((E >> lane) & 1ull) {
            const uint32_t k = ends + (uint32_t)__popcll(E & below);
            if (k < kTokenMaxCount) s_tok[k] |= (i - s_tok[k]) << 16;
        }
        count += (uint32_t)__popcll(S);
        ends += (uint32_t)__popcll(E);
        kept += (uint32_t)__popcll(K);
    }
    count = min(count, kTokenMaxCount);  // (a span of m characters holds at most (m + 1) / 2 tokens)
    __syncthreads();
    if (A.len_out) {
        if (lane == 0) A.len_out[q] = count ? kept + count - 1u : 0u;
        return;
    }

    // order the table
    if (count <= 64) {
        const uint32_t e = lane < count ? s_tok[lane] : kTokPad;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < count; ++j) rank += tok_less<kStored>(s_chars, s_valid, s_tok[j], e) ? 1u : 0u;
        __syncthreads();
        if (lane < count) s_tok[rank] = e;
        __syncthreads();
    } else {
        uint32_t n2 = 128;
        while (n2 < count) n2 <<= 1;
        for (uint32_t i = count + lane; i < n2; i += 64) s_tok[i] = kTokPad;
        __syncthreads();
        for (uint32_t k2 = 2; k2 <= n2; k2 <<= 1)
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (uint32_t i = lane; i < n2; i += 64) {
                    const uint32_t p = i ^ j;
                    if (p > i) {
                        const uint32_t a = s_tok[i], b = s_tok[p];
                        if (tok_less<kStored>(s_chars, s_valid, b, a) == ((i & k2) == 0)) {
                            s_tok[i] = b;
                            s_tok[p] = a;
                        }
                    }
                }
                __syncthreads();
            }
    }

    // output positions: the exclusive sums of (length + 1) in sorted order
    uint32_t run = 0;
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t k = base + lane;
        const uint32_t len1 = k < count ? (s_tok[k] >> 16) + 1u : 0u;
        uint32_t incl = len1;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += t;
        }
        if (k < count) s_pos[k] = (uint16_t)(run + incl - len1);
        run += (uint32_t)__shfl((int)incl, 63);
    }
    const uint32_t total = count ? run - 1u : 0u;  // <= m
    __syncthreads();

    // every output character: the last sorted token that starts at or in front of it, or a blank
    const uint64_t nout = kStored ? total : n;
    for (uint64_t p = lane; p < nout; p += 64) {
        uint32_t c = (uint32_t)' ';
        if (p < total) {
            uint32_t lo = 0, hi = count - 1u;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1u) >> 1;
                if (s_pos[mid] <= (uint32_t)p) lo = mid;
                else hi = mid - 1u;
            }
            const uint32_t e = s_tok[lo], o = (uint32_t)p - s_pos[lo];
            if (o < (e >> 16)) c = s_chars[(e & 0xFFFFu) + o];
        }
        out[p] = (CharT)c;
    }
    if (!kStored && kWide && out != in && lane < ((qe - qa) & 3u))  // bytes behind the last whole character
        A.out[qa + n * cs + lane] = A.raw[qa + n * cs + lane];
}

template <bool kStored>
void launch_token_as(uint32_t cs, const TokenArgs& A, hipStream_t s) {
    if (cs == 4) hipLaunchKernelGGL((k_token_sort<true, kStored>), dim3(A.n), dim3(64), 0, s, A);
    else hipLaunchKernelGGL((k_token_sort<false, kStored>), dim3(A.n), dim3(64), 0, s, A);
}

}  // namespace

hipError_t launch_token_sort(const uint32_t valid[8], uint32_t cs, const uint8_t* raw, const uint64_t* off, uint32_t n,
                             uint8_t* out, hipStream_t s) {
    if (!n) return hipSuccess;
    TokenArgs A{raw, off, out, off, nullptr, n, {}};
    for (int i = 0; i < 8; ++i) A.V.w[i] = valid[i];
    launch_token_as<false>(cs, A, s);
    return hipGetLastError();
}

hipError_t sorted_term_offsets(const DevIndex& X, uint64_t* ts_off, hipStream_t s) {
    const uint32_t n = X.n_terms;
    if (!n) return hipMemsetAsync(ts_off, 0, sizeof(uint64_t), s);
    size_t scan_bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                    (int)n + 1);
    if (e != hipSuccess) return e;
    const size_t len_bytes = (sizeof(uint64_t) * ((size_t)n + 1) + 255) / 256 * 256;
    uint8_t* temp = nullptr;  // [lengths u64 (n + 1) | the scan's scratch]
    if ((e = hipMalloc(&temp, len_bytes + scan_bytes)) != hipSuccess) return e;
    uint64_t* len = reinterpret_cast<uint64_t*>(temp);
    e = hipMemsetAsync(len + n, 0, sizeof(uint64_t), s);
    if (e == hipSuccess) {
        TokenArgs A{X.term_bytes, X.term_off, nullptr, nullptr, len, n, {}};
        launch_token_as<true>(X.csize, A, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(temp + len_bytes, scan_bytes, len, ts_off, (int)n + 1, s);
    const hipError_t w = hipStreamSynchronize(s);
    (void)hipFree(temp);
    return e != hipSuccess ? e : w;
}

hipError_t launch_sorted_terms(const DevIndex& X, const uint64_t* ts_off, uint8_t* ts_bytes, hipStream_t s) {
    if (!X.n_terms) return hipSuccess;
    TokenArgs A{X.term_bytes, X.term_off, ts_bytes, ts_off, nullptr, X.n_terms, {}};
    launch_token_as<true>(X.csize, A, s);
    return hipGetLastError();
}

}  // namespace ngs
