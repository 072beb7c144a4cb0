// ngs_join.hip — the stages around ngsSearchDevice that turn "the library against itself" into one
// device-side pipeline, for gfx950.
//
// k_key_queries   the keys [first, first + n) as a query batch: offsets from key_off by formula, the
//                 bytes as a segmented gather (a thread owns 16 output bytes);
// k_shift_offsets a batch's offsets moved up by a constant: the keys of several indexes in one batch (§9.8);
// k_drop_self     one wave per row: the row's own record found by ballot, the later records moved up
//                 in chunks of 64, the row cut to the limit;
// k_keep_similar  one wave per row: the records with sim >= min_sim kept in order (dedupKeys);
// k_union / k_labels / k_label_init   a lock-free union-find over the block's (key, key) records.
#include <hip/hip_runtime.h>

#include "ngs_common.h"
#include "ngs_join.h"

namespace ngs {
namespace {

// ---- gather ----
// Thread t owns the 16 bytes at "virtual" positions [16 t, 16 t + 16), where position v is output byte
// v - mis and mis = the output pointer's misalignment from 16: a thread's bytes are one aligned
// 16-byte store when they all exist, dword or byte stores at the batch's two ends. The key of its
// first byte comes from a binary search of the offset formula; within a key the source is the
// output shifted by a constant, read as aligned dwords and funnel-shifted on a narrow index (a key
// starts at any byte), one dword per character on a wide one. Only dwords holding a needed byte are
// loaded: the last of them may end up to two bytes past the keys' last NUL, inside the dword of
// padding key_bytes is uploaded with. A batch without bytes (n = 0, or empty keys only) reads
// nothing but key_off[first .. first + n].
template <bool kWide>
__global__ __launch_bounds__(256) void k_key_queries(const uint64_t* __restrict__ key_off,
                                                     const uint8_t* __restrict__ key_bytes, uint32_t first, uint32_t n,
                                                     uint64_t total, uint8_t* __restrict__ out,
                                                     uint64_t* __restrict__ off, uint32_t mis) {
    constexpr uint32_t cs = kWide ? 4u : 1u;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t k0 = key_off[first];
    auto qoff = [&](uint32_t i) { return (key_off[first + i] - k0 - i) * cs; };
    if (t <= n) off[t] = qoff((uint32_t)t);
    const uint64_t v0 = t * 16u, vend = (uint64_t)mis + total;
    if (total == 0 || v0 >= vend) return;  // (no bytes: qoff(i + 1) below would read past key_off when n = 0)

    // the key holding this thread's first byte: the last i with qoff(i) <= b (empty keys share an offset)
    const uint64_t b0 = v0 < mis ? 0 : v0 - mis;
    uint32_t lo = 0, hi = n;  // qoff(lo) <= b0 < qoff(hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (qoff(mid) <= b0) lo = mid;
        else hi = mid;
    }
    uint32_t i = lo;
    uint64_t end = qoff(i + 1u);         // output bytes of key i end here
    uint64_t shift = (k0 + i) * cs;      // source byte = output byte + shift
    auto seek = [&](uint64_t b) {        // b ascends from call to call and is < total
        while (b >= end) {
            ++i;
            end = qoff(i + 1u);
            shift = (k0 + i) * cs;
        }
    };

    uint32_t w[4];
    bool whole[4];
    uint8_t* vbase = out - mis;  // 16-byte aligned
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
        const uint64_t v = v0 + 4u * d;
        whole[d] = v >= mis && v + 4u <= vend;
        w[d] = 0;
        if (whole[d]) {
            const uint64_t b = v - mis;
            seek(b);
            if (b + 4u <= end) {  // the dword lies in one key
                const uint64_t src = b + shift;
                const uint32_t* a = reinterpret_cast<const uint32_t*>(key_bytes + (src & ~(uint64_t)3));
                const uint32_t sh = kWide ? 0u : (uint32_t)(src & 3u);
                w[d] = sh ? (a[0] >> (8u * sh)) | (a[1] << (32u - 8u * sh)) : a[0];
            } else {
                for (uint32_t e = 0; e < 4; ++e) {
                    seek(b + e);
                    w[d] |= (uint32_t)key_bytes[b + e + shift] << (8u * e);
                }
            }
        } else {  // an end of the batch: the bytes that exist, one by one
            for (uint32_t e = 0; e < 4; ++e) {
                const uint64_t ve = v + e;
                if (ve < mis || ve >= vend) continue;
                seek(ve - mis);
                vbase[ve] = key_bytes[ve - mis + shift];
            }
        }
    }
    if (whole[0] && whole[1] && whole[2] && whole[3]) {
        *reinterpret_cast<uint4*>(vbase + v0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d)
            if (whole[d]) *reinterpret_cast<uint32_t*>(vbase + v0 + 4u * d) = w[d];
    }
}

// off[i] += add for i < n: a gather of several indexes' keys into one batch (launch_shift_offsets)
__global__ __launch_bounds__(256) void k_shift_offsets(uint64_t* __restrict__ off, uint64_t n, uint64_t add) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) off[i] += add;
}

// ---- drop-self ----
constexpr uint32_t kRowsPerBlock = 4;  // one wave per row

__global__ __launch_bounds__(64 * kRowsPerBlock) void k_drop_self(uint32_t* counts, uint32_t* keys, float* scores,
                                                                 uint32_t n, uint32_t stride, uint32_t first,
                                                                 uint32_t limit) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const uint32_t count = min(counts[row], stride);
    const uint64_t self = (uint64_t)first + row;
    uint32_t* k = keys + row * stride;
    float* sc = scores + row * stride;
    // the row's own record: at most one, anywhere
    uint32_t p = count;
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t r = base + lane;
        const uint64_t hit = __ballot(r < count && (uint64_t)k[r] == self);
        if (hit) {
            p = base + (uint32_t)__ffsll((unsigned long long)hit) - 1u;
            break;
        }
    }
    const uint32_t kept = join_row_count(count, p < count, limit);
    // cells [p, kept) take their right neighbours, a chunk of 64 at a time in ascending order. A
    // chunk's last lane reads the next chunk's first cell; that chunk is stored only in the next
    // iteration, after this one's loads have returned (the stores below consume them, and the
    // explicit wait keeps it so whatever the compiler does with the loop).
    for (uint32_t base = p & ~63u; base < kept; base += 64) {
        const uint32_t r = base + lane;
        const bool mine = r >= p && r < kept;  // r + 1 <= kept <= count - 1 < stride
        const uint32_t nk = mine ? k[r + 1] : 0u;
        const float ns = mine ? sc[r + 1] : 0.0f;
        __builtin_amdgcn_s_waitcnt(0);
        if (mine) {
            k[r] = nk;
            sc[r] = ns;
        }
    }
    if (lane == 0) counts[row] = kept;
}

// the records with sim >= min_sim, in order (what ngsRerankDevice keeps, without its sort and
// without its cap on the stride: a join row's stride is one more than the limit)
// (kMoveSim: the similarities move with their records, in place; sim is then written too)
template <bool kMoveSim>
__global__ __launch_bounds__(64 * kRowsPerBlock) void k_keep_similar(uint32_t* counts, uint32_t* keys, float* scores,
                                                                    const float* sim, float* sim_out, uint32_t n,
                                                                    uint32_t stride, float min_sim) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const uint32_t count = min(counts[row], stride);
    uint32_t* k = keys + row * stride;
    float* sc = scores + row * stride;
    const float* sv = sim + row * stride;
    uint32_t kept = 0;  // every chunk writes at or below the cells it read
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t r = base + lane;
        const bool live = r < count;
        const uint32_t rk = live ? k[r] : 0u;
        const float rs = live ? sc[r] : 0.0f;
        const float rv = live ? sv[r] : 0.0f;
        const bool keep = live && !(rv < min_sim);
        const uint64_t bal = __ballot(keep);
        const uint32_t at = kept + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        __builtin_amdgcn_s_waitcnt(0);
        if (keep) {
            k[at] = rk;
            sc[at] = rs;
            if (kMoveSim) sim_out[row * stride + at] = rv;
        }
        kept += (uint32_t)__popcll(bal);
    }
    if (lane == 0) counts[row] = kept;
}

// ---- cluster ----
// labels[] is a forest with labels[x] <= x. Cells other waves may be rewriting are read and written
// as relaxed device-scope atomics. A cell leaves the state "root" (labels[x] == x) once, by the
// compare-and-swap of a hook, and only ever moves to smaller ancestors afterwards, so whatever
// value a find reads is an ancestor of x: path halving may race with itself and with hooks.
__device__ __forceinline__ uint32_t ld_label(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_label(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t find_root(uint32_t* labels, uint32_t x) {
    for (;;) {  // every step moves to a smaller id
        const uint32_t p = ld_label(labels + x);
        if (p == x) return x;
        const uint32_t gp = ld_label(labels + p);
        if (gp != p) st_label(labels + x, gp);
        x = gp;
    }
}

__global__ __launch_bounds__(256) void k_label_init(uint32_t* __restrict__ labels, uint32_t n_labels) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x < n_labels) labels[x] = x;
}

// A group of g = 2^lg lanes per row (g the stride rounded up to a power of two, 64 at the most): a
// lane takes the row's records r = its place in the group, + g, ... below the count. The launch is
// n x g threads whatever the stride, and no thread divides.
__global__ __launch_bounds__(256) void k_union(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ keys,
                                               uint32_t n, uint32_t stride, uint32_t first, uint32_t* labels,
                                               uint32_t n_labels, uint32_t lg) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = t >> lg;
    if (row >= n) return;
    const uint64_t self = (uint64_t)first + row;
    if (self >= n_labels) return;  // nothing is read through such an id
    const uint32_t count = min(counts[row], stride);
    const uint32_t* k = keys + row * stride;
    for (uint32_t r = (uint32_t)t & ((1u << lg) - 1u); r < count; r += 1u << lg) {
        uint32_t a = (uint32_t)self, b = k[r];
        if (b >= n_labels) continue;
        for (;;) {
            a = find_root(labels, a);
            b = find_root(labels, b);
            if (a == b) break;
            const uint32_t hi = max(a, b), lo = min(a, b);
            // hook on the root's own cell: fails only if another wave hooked `hi` first, which made
            // the forest smaller, so the retries end
            if (atomicCAS(labels + hi, hi, lo) == hi) break;
            a = hi;
            b = lo;
        }
    }
}

// a launch of its own behind the unions: the roots are fixed, and a racing labels[x] = root only
// shortens someone else's path
__global__ __launch_bounds__(256) void k_labels(uint32_t* labels, uint32_t n_labels) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= n_labels) return;
    uint32_t r = x;
    for (;;) {
        const uint32_t p = ld_label(labels + r);
        if (p == r) break;
        r = p;
    }
    st_label(labels + x, r);
}

}  // namespace

hipError_t launch_key_queries(const DevIndex& X, uint32_t first, uint32_t n, uint64_t total, uint8_t* bytes,
                              uint64_t* off, hipStream_t s) {
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(bytes) & 15u);
    const uint64_t chunks = total ? (mis + total + 15u) / 16u : 0;
    const uint64_t threads = chunks > (uint64_t)n + 1u ? chunks : (uint64_t)n + 1u;
    const uint64_t blocks = (threads + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (X.csize == 4)
        hipLaunchKernelGGL(k_key_queries<true>, dim3((uint32_t)blocks), dim3(256), 0, s, X.key_off, X.key_bytes, first,
                           n, total, bytes, off, mis);
    else
        hipLaunchKernelGGL(k_key_queries<false>, dim3((uint32_t)blocks), dim3(256), 0, s, X.key_off, X.key_bytes, first,
                           n, total, bytes, off, mis);
    return hipGetLastError();
}

hipError_t launch_shift_offsets(uint64_t* off, uint64_t n, uint64_t add, hipStream_t s) {
    if (!n || !add) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_shift_offsets, dim3((uint32_t)blocks), dim3(256), 0, s, off, n, add);
    return hipGetLastError();
}

hipError_t launch_drop_self(uint32_t* counts, uint32_t* keys, float* scores, uint32_t n, uint32_t stride,
                            uint32_t first, uint32_t limit, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_drop_self, dim3((n + kRowsPerBlock - 1u) / kRowsPerBlock), dim3(64 * kRowsPerBlock), 0, s,
                       counts, keys, scores, n, stride, first, limit);
    return hipGetLastError();
}

hipError_t launch_keep_similar(uint32_t* counts, uint32_t* keys, float* scores, const float* sim, uint32_t n,
                               uint32_t stride, float min_sim, hipStream_t s, float* sim_out) {
    if (!n) return hipSuccess;
    const dim3 grid((n + kRowsPerBlock - 1u) / kRowsPerBlock), block(64 * kRowsPerBlock);
    if (sim_out)
        hipLaunchKernelGGL(k_keep_similar<true>, grid, block, 0, s, counts, keys, scores, sim, sim_out, n, stride, min_sim);
    else
        hipLaunchKernelGGL(k_keep_similar<false>, grid, block, 0, s, counts, keys, scores, sim, sim_out, n, stride,
                           min_sim);
    return hipGetLastError();
}

hipError_t launch_cluster(const uint32_t* counts, const uint32_t* keys, uint32_t n, uint32_t stride, uint32_t first,
                          uint32_t* labels, uint32_t n_labels, uint32_t flags, hipStream_t s) {
    if (!n_labels) return hipSuccess;
    const uint32_t lblocks = (uint32_t)(((uint64_t)n_labels + 255u) / 256u);
    if (flags & kClusterInit) {
        hipLaunchKernelGGL(k_label_init, dim3(lblocks), dim3(256), 0, s, labels, n_labels);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (n && stride) {
        uint32_t lg = 0;
        while (lg < 6u && (1u << lg) < stride) ++lg;
        const uint64_t blocks = (((uint64_t)n << lg) + 255u) / 256u;
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_union, dim3((uint32_t)blocks), dim3(256), 0, s, counts, keys, n, stride, first, labels,
                           n_labels, lg);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (flags & kClusterFinish) {
        hipLaunchKernelGGL(k_labels, dim3(lblocks), dim3(256), 0, s, labels, n_labels);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace ngs
