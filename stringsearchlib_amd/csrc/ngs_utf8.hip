// ngs_utf8.hip — device UTF-8 decoder for gfx950: a batch of UTF-8 queries in HBM becomes the
// UTF-32 batch (bytes + byte offsets) that k_prep and everything behind it take.
//
// Three steps on one stream: k_utf8_count (units per query), an exclusive scan of the counts
// (hipcub, as launch_pack), k_utf8_write (the units, and the output offsets in bytes). The
// decoding rule is local (ngs_utf8.h: utf8_starts), so both kernels run one lane per byte.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ngs_utf8.h"

namespace ngs {
namespace {

// Shaped as k_prep: queries are tens of bytes, so four queries per wave, 16 lanes each. A query is
// walked in 16-byte windows; the wave's ballot of "a unit starts at my byte", cut to the group's 16
// bits, gives each starting lane its write index (the popcount below the lane) and the window's
// unit count, which `run` carries to the next window in a register. A lane reads its byte's
// neighbours (up to 3 back to the lead, up to 3 on from it) with plain global loads that L1
// serves; utf8_starts / utf8_wf_len stop at the query's own first and last byte, so a lead byte
// that ends query q never takes in the continuation bytes that open query q + 1. The window loop
// runs while any query of the wave has bytes left, so every ballot sees the whole wave.
template <bool kWrite>
__device__ __forceinline__ uint32_t utf8_walk(const uint8_t* __restrict__ s, uint64_t len, uint32_t gl, uint32_t sh,
                                              uint32_t* __restrict__ dst, uint32_t cap) {
    uint32_t run = 0;
    for (uint64_t base = 0; __ballot(base < len); base += 16) {
        const uint64_t i = base + gl;
        const bool st = i < len && utf8_starts(s, len, i);
        const uint32_t bal = (uint32_t)(__ballot(st) >> sh) & 0xFFFFu;
        if (kWrite && st) {
            const uint32_t idx = run + __popc(bal & ((1u << gl) - 1u));
            if (idx < cap) dst[idx] = utf8_unit(s + i, utf8_wf_len(s + i, len - i));
        }
        run += __popc(bal);
    }
    return run;
}

// query q's bytes: absolute offsets; a descending pair reads as an empty query
__device__ __forceinline__ uint64_t query_span(const uint64_t* __restrict__ off, uint32_t q, uint64_t& a) {
    a = off[q];
    const uint64_t e = off[q + 1];
    return e > a ? e - a : 0;
}

__global__ __launch_bounds__(64) void k_utf8_count(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ off,
                                                   uint32_t n, uint32_t* __restrict__ cnt) {
    const uint32_t lane = threadIdx.x, gl = lane & 15u, sh = lane & 48u;
    const uint32_t q = blockIdx.x * 4 + (lane >> 4);
    uint64_t a = 0;
    const uint64_t len = q < n ? query_span(off, q, a) : 0;
    const uint32_t units = utf8_walk<false>(raw + a, len, gl, sh, nullptr, 0);
    if (q < n && gl == 0) cnt[q] = units;
    if (blockIdx.x == 0 && lane == 0) cnt[n] = 0;  // the scan runs over n + 1 items: scan[n] = total
}

// scan[0 .. n]: exclusive prefix sum of the counts, in units. Query q is kept when it ends within
// cap units; the kept queries are a prefix of the batch (the sums ascend), K units in all, and every
// query past them is empty at offset K.
__global__ __launch_bounds__(64) void k_utf8_write(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ off,
                                                   uint32_t n, const uint32_t* __restrict__ cnt,
                                                   const uint64_t* __restrict__ scan, uint64_t cap,
                                                   uint32_t* __restrict__ out, uint64_t* __restrict__ out_off) {
    const uint32_t lane = threadIdx.x, gl = lane & 15u, sh = lane & 48u;
    const uint32_t q = blockIdx.x * 4 + (lane >> 4);
    const bool live = q < n;
    uint64_t a = 0, len = 0, at = 0;
    uint32_t c = 0;
    bool keep = false;
    if (live) {
        at = scan[q];
        c = cnt[q];
        keep = at + c <= cap;
        if (keep) len = query_span(off, q, a);
        if (gl == 0) {
            const uint64_t total = scan[n];
            uint64_t kept = total;
            if (total > cap) {  // the first query d with scan[d + 1] > cap: K = scan[d]
                uint32_t lo = 0, hi = n - 1;
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (scan[mid + 1] > cap) hi = mid; else lo = mid + 1;
                }
                kept = scan[lo];
            }
            out_off[q] = 4 * (keep ? at : kept);
            if (q == n - 1) out_off[n] = 4 * kept;
        }
    }
    utf8_walk<true>(raw + a, len, gl, sh, out + (keep ? at : 0), keep ? c : 0u);
}

struct UnitsToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};
using CountIter = hipcub::TransformInputIterator<uint64_t, UnitsToU64, const uint32_t*>;

constexpr size_t kAlign = 256;
size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }
size_t scan_temp_bytes(uint32_t n) {
    size_t bytes = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, CountIter((const uint32_t*)nullptr, UnitsToU64()),
                                     (uint64_t*)nullptr, (int)n + 1);
    return bytes;
}

}  // namespace

// temp: [counts u32 (n + 1) | sums u64 (n + 1) | the scan's scratch]
size_t utf8_temp_bytes(uint32_t n) {
    return align_up(sizeof(uint32_t) * ((size_t)n + 1)) + align_up(sizeof(uint64_t) * ((size_t)n + 1)) +
           align_up(scan_temp_bytes(n));
}

hipError_t launch_utf8_decode(const uint8_t* raw8, const uint64_t* off8, uint32_t n, uint32_t* out32,
                              uint64_t out_cap_units, uint64_t* out_off, void* temp, size_t temp_bytes,
                              hipStream_t stream) {
    if (n == 0) return hipMemsetAsync(out_off, 0, sizeof(uint64_t), stream);
    if (n >= 0x7FFFFFFFu || !temp || temp_bytes < utf8_temp_bytes(n)) return hipErrorInvalidValue;
    uint8_t* t = static_cast<uint8_t*>(temp);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(t);
    t += align_up(sizeof(uint32_t) * ((size_t)n + 1));
    uint64_t* scan = reinterpret_cast<uint64_t*>(t);
    t += align_up(sizeof(uint64_t) * ((size_t)n + 1));
    size_t sbytes = temp_bytes - (size_t)(t - static_cast<uint8_t*>(temp));
    const dim3 grid((n + 3) / 4), block(64);
    hipLaunchKernelGGL(k_utf8_count, grid, block, 0, stream, raw8, off8, n, cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(t, sbytes, CountIter(cnt, UnitsToU64()), scan, (int)n + 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_utf8_write, grid, block, 0, stream, raw8, off8, n, (const uint32_t*)cnt,
                       (const uint64_t*)scan, out_cap_units, out32, out_off);
    return hipGetLastError();
}

}  // namespace ngs
