// ngs_sim.hip — the verification stage behind the search: the edit-distance
// similarity of every (query, key) record of a result block, and the re-rank by it, for gfx950.
//
// sim_wave: one wave per query, the body of both similarity kernels. The wave normalises the query
// as k_prep does (ballot windows find the trim), then takes one of two wave-uniform paths by the
// normalised length m:
//   m <= 64   lanes are records: the query's match masks go to LDS once, and every lane follows
//             key -> term -> term_off -> term_bytes and streams its term through the one-word global
//             Myers recurrence (ngs_sim.h: myers_step with hin = +1);
//   m <= 4096 one record at a time, the wave as a systolic pipeline: lane w holds query word w
//             (its 64 characters in registers) and takes the horizontal delta lane w - 1 produced
//             one step earlier.
// k_rerank: one workgroup per query sorts (sim desc, position asc) in LDS and permutes in place.
// The metric (ngs_sim.h: Levenshtein, OSA, partial) and the matched-term output are template
// parameters of the body, the term array one of k_rerank: the launch functions pick
// the instantiation; the entry points without a metric are kSimLevenshtein, no terms.
// The body takes the arrays behind a key id from a source, and each source has its
// kernel: k_sim, one index held in registers, and k_sim_set, an index set whose member of every
// record is looked up in the wave, in a table in LDS.
#include <hip/hip_runtime.h>

#include "ngs_common.h"
#include "ngs_set.h"
#include "ngs_sim.h"

namespace ngs {
namespace {

struct SimArgs {
    const uint8_t* raw;
    const uint64_t* off;
    const uint32_t* counts;
    const uint32_t* keys;
    float* sim;
    uint32_t* terms;           // kTerms: the matched term ids, in sim's layout
    const uint32_t* key_term;  // indexes without kt_off: the term of each key
    uint32_t n, stride;
    ValidSet V;
};

__device__ __forceinline__ uint32_t ld_char(const uint8_t* base, uint64_t i, uint32_t cs) {
    return cs == 4 ? reinterpret_cast<const uint32_t*>(base)[i] : (uint32_t)base[i];
}

// the terms of M's local key `key`: [j, je) of kt_term, or the one term of key_term (j = 0, je = 1)
__device__ __forceinline__ void key_terms(const SimMember& M, uint32_t key, uint32_t& j, uint32_t& je) {
    if (M.kt_off) {
        j = M.kt_off[key];
        je = M.kt_off[key + 1];
    } else {
        j = 0;
        je = 1;
    }
}
__device__ __forceinline__ uint32_t term_at(const SimMember& M, uint32_t key, uint32_t j) {
    return M.kt_off ? M.kt_term[j] : M.key_term[key];
}

// Where a key id's arrays come from: total key ids, member(g) the index owning g < total, at(p) its
// arrays with the first key id it owns. One index is a SimMember in registers: nothing is looked up,
// and its base of 0 and the member index fold away.
struct OneIndex {
    SimMember M;
    uint32_t total;
    __device__ __forceinline__ uint32_t member(uint32_t) const { return 0; }
    __device__ __forceinline__ const SimMember& at(uint32_t) const { return M; }
};
// An index set: the members' descriptors in LDS, so that lanes in different members
// index them without a trip to memory. Their bases ascend from 0: the owner of g is the last member
// whose base is at or below it. Members with kt_off / kt_term and with the key_term map mix freely.
struct IndexSet {
    const SimMember* m;
    uint32_t P, total;
    __device__ __forceinline__ uint32_t member(uint32_t g) const {
        uint32_t p = 0;
        for (uint32_t i = 1; i < P; ++i) p += m[i].base <= g ? 1u : 0u;
        return p;
    }
    __device__ __forceinline__ const SimMember& at(uint32_t p) const { return m[p]; }
};

// The recurrence's state and one column of it by metric (ngs_sim.h): kSimOsa carries two more words
// and the transposition bit between blocks; kSimPartial is the Levenshtein step behind hin = 0.
template <uint32_t kMetric>
struct SimBlock : MyersBlock {};
template <>
struct SimBlock<kSimOsa> : OsaBlock {};
template <uint32_t kMetric>
__device__ __forceinline__ int sim_step(SimBlock<kMetric>& b, uint64_t eq, int hin, uint32_t tin, uint64_t top,
                                        uint32_t& tout) {
    if constexpr (kMetric == kSimOsa) return osa_step(b, eq, hin, tin, top, tout);
    else return myers_step(b, eq, hin, top);
}
template <uint32_t kMetric>
constexpr int kSimTopDelta = kMetric == kSimPartial ? 0 : +1;  // the horizontal delta of row 0
// the score after a column: kSimPartial keeps the least over the columns in `low`
template <uint32_t kMetric>
__device__ __forceinline__ void sim_column(uint32_t& score, uint32_t& low, int hout) {
    score += (uint32_t)hout;
    if constexpr (kMetric == kSimPartial) low = min(low, score);
}
template <uint32_t kMetric>
__device__ __forceinline__ float sim_of(uint32_t d, uint32_t m, uint32_t L) {
    if constexpr (kMetric == kSimPartial) return sim_value_partial(d, m);
    else return sim_value(d, m, L);
}

// d(Q, T) of a narrow term through the byte-indexed mask table: the term is read a dword at a
// time with the next one in flight, as myers_match_t does (term_bytes is padded by two dwords)
template <uint32_t kMetric>
__device__ __forceinline__ uint32_t myers_narrow(const uint64_t* peq, uint32_t m, const uint8_t* tb, uint64_t a,
                                                 uint32_t L) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(tb + (a & ~(uint64_t)3));
    const uint32_t skip = (uint32_t)(a & 3u);
    uint32_t cur = w[0] >> (8u * skip), nxt = skip + L > 4u ? w[1] : 0u;
    uint32_t avail = 4u - skip, k = 1, score = m, low = m, tout = 0;
    const uint64_t top = 1ull << (m - 1u);
    SimBlock<kMetric> b;
    for (uint32_t j = 0; j < L; ++j) {
        if (!avail) {
            cur = nxt;
            avail = 4u;
            ++k;
            if (j + 4u < L) nxt = w[k];
        }
        const uint32_t c = cur & 255u;
        cur >>= 8;
        --avail;
        sim_column<kMetric>(score, low, sim_step<kMetric>(b, peq[c], kSimTopDelta<kMetric>, 0u, top, tout));
    }
    return kMetric == kSimPartial ? low : score;
}

// the wide table: kSimSlots masks, then kSimSlots keys; a character not in it matches no row
__device__ __forceinline__ uint64_t wide_mask(const uint64_t* mask, const uint32_t* slot_key, uint32_t c) {
    uint32_t s = sim_slot(c);
    for (;;) {
        const uint32_t k = slot_key[s];
        if (k == c) return mask[s];
        if (k == kSimEmpty) return 0;
        s = (s + 1u) & (kSimSlots - 1u);
    }
}
template <uint32_t kMetric>
__device__ __forceinline__ uint32_t myers_wide(const uint64_t* mask, const uint32_t* slot_key, uint32_t m,
                                               const uint32_t* t, uint32_t L) {
    const uint64_t top = 1ull << (m - 1u);
    SimBlock<kMetric> b;
    uint32_t score = m, low = m, tout = 0, nxt = t[0];
    for (uint32_t j = 0; j < L; ++j) {
        const uint32_t c = nxt;
        if (j + 1u < L) nxt = t[j + 1u];
        sim_column<kMetric>(score, low,
                            sim_step<kMetric>(b, wide_mask(mask, slot_key, c), kSimTopDelta<kMetric>, 0u, top, tout));
    }
    return kMetric == kSimPartial ? low : score;
}

// a record's best term so far: the larger similarity, and with kTerms the smaller term id among equals
template <bool kTerms>
__device__ __forceinline__ void sim_take(float& best, uint32_t& best_t, float v, uint32_t t) {
    if constexpr (kTerms) {
        if (v > best || (v == best && t < best_t)) {
            best = v;
            best_t = t;
        }
    } else {
        best = fmaxf(best, v);
    }
}

// One wave's work on query blockIdx.x, for both kernels: everything but where a key id's arrays
// come from, which is `src`. The barrier behind s_valid also orders what the caller wrote to LDS
// before the call (k_sim_set's member table).
template <bool kWide, uint32_t kMetric, bool kTerms, class Src>
__device__ __forceinline__ void sim_wave(const Src& src, const SimArgs& A) {
    constexpr uint32_t cs = kWide ? 4u : 1u;
    __shared__ uint64_t s_mask[256];             // narrow: by byte; wide: slots [0, kSimSlots)
    __shared__ uint32_t s_key[kSimSlots];        // wide: the slots' characters
    __shared__ uint32_t s_valid[8];
    const uint32_t lane = threadIdx.x, q = blockIdx.x;
    if (lane < 8) s_valid[lane] = A.V.w[lane];
    __syncthreads();  // (the workgroup is one wave: the barriers here order its LDS accesses only)

    const uint32_t count = min(A.counts[q], A.stride);
    if (count == 0) return;
    const uint32_t* keys = A.keys + (size_t)q * A.stride;
    float* out = A.sim + (size_t)q * A.stride;
    uint32_t* out_t = kTerms ? A.terms + (size_t)q * A.stride : nullptr;
    const uint64_t qa = A.off[q], qe = A.off[q + 1];
    const uint64_t n = qe > qa ? (qe - qa) / cs : 0;
    const uint8_t* rq = A.raw + qa;

    // wildcard, trim, length: everything here is uniform over the wave
    float fixed = 0.0f;
    bool is_fixed = false;
    uint64_t first = n, m64 = 0;
    if (n == 0 || (n == 1 && ld_char(rq, 0, cs) == (uint32_t)'*')) {
        fixed = kSimWildcard;
        is_fixed = true;
    } else {
        for (uint64_t base = 0; base < n; base += 64) {
            const uint64_t i = base + lane;
            const uint64_t bal = __ballot(i < n && sim_keeps(s_valid, ld_char(rq, i, cs), cs));
            if (bal) {
                first = base + (uint32_t)__ffsll((unsigned long long)bal) - 1u;
                break;
            }
        }
        if (first < n) {
            uint64_t last = first;
            for (uint64_t base = 0; base < n; base += 64) {
                const uint64_t i = base + lane;
                const uint64_t bal = __ballot(i < n && sim_keeps(s_valid, ld_char(rq, n - 1 - i, cs), cs));
                if (bal) {
                    last = n - 1 - (base + (uint32_t)__ffsll((unsigned long long)bal) - 1u);
                    break;
                }
            }
            m64 = last - first + 1;
        }
        if (m64 > kSimMaxQuery) {
            fixed = kSimNone;
            is_fixed = true;
        }
    }
    if (is_fixed) {
        for (uint32_t r = lane; r < count; r += 64) {
            out[r] = fixed;
            if constexpr (kTerms) out_t[r] = kSimNoTerm;
        }
        return;
    }
    const uint32_t m = (uint32_t)m64;
    const uint8_t* nq = rq + first * cs;  // Q[i] = sim_norm(nq[i])

    if (m <= 64) {
        // ---- short path: match masks in LDS, lanes are records ----
        const uint32_t qc = lane < m ? sim_norm(s_valid, ld_char(nq, lane, cs), cs) : kSimEmpty;
        uint64_t mine = 0;  // the rows holding this lane's character
        for (uint32_t i = 0; i < m; ++i) mine |= __shfl(qc, (int)i) == qc ? 1ull << i : 0ull;
        if (kWide) {
            s_key[lane] = kSimEmpty;
            s_key[lane + 64] = kSimEmpty;
        } else {
            for (uint32_t i = lane; i < 256; i += 64) s_mask[i] = 0;
        }
        __syncthreads();
        if (lane < m) {
            if (!kWide) {
                s_mask[qc] = mine;  // (lanes of one character store one value)
            } else if ((uint32_t)__ffsll((unsigned long long)mine) - 1u == lane) {  // a character's first row inserts it
                uint32_t s = sim_slot(qc);
                for (;;) {
                    const uint32_t old = atomicCAS(&s_key[s], kSimEmpty, qc);
                    if (old == kSimEmpty || old == qc) break;
                    s = (s + 1u) & (kSimSlots - 1u);
                }
                s_mask[s] = mine;
            }
        }
        __syncthreads();

        // a record's place in its index: the member p, the local key, the terms [j, je) still to
        // compare and the first of them, tt = [ta, tb) (tt is read with kTerms). A key id at or past
        // src.total has none, and nothing is read through it.
        struct Rec {
            uint32_t p, key, j, je, tt;
            uint64_t ta, tb;
        };
        auto first_term = [&](uint32_t g) {
            Rec f{0, g, 0, 0, kSimNoTerm, 0, 0};  // (the key starts as the id: see the long path)
            if (g >= src.total) return f;
            f.p = src.member(g);
            const SimMember& M = src.at(f.p);
            f.key = g - M.base;
            if (f.key >= M.n_keys) return f;
            key_terms(M, f.key, f.j, f.je);
            if (f.j >= f.je) return f;
            const uint32_t t = term_at(M, f.key, f.j);
            if (t >= M.n_terms) return f;
            f.tt = t;
            f.ta = M.term_off[t];
            f.tb = M.term_off[t + 1];
            return f;
        };
        // rounds of 64 records; the next round's member -> key -> term -> offsets chain is issued
        // before the current round's recurrence
        Rec c = first_term(lane < count ? keys[lane] : kSimEmpty);
        for (uint32_t base = 0; base < count; base += 64) {
            const uint32_t r = base + lane, rn = r + 64;
            const Rec nx = first_term(rn < count ? keys[rn] : kSimEmpty);
            const SimMember& M = src.at(c.p);
            float best = kSimNone;
            uint32_t best_t = kSimNoTerm;
            while (c.j < c.je) {
                if (c.tb > c.ta) {
                    const uint32_t L = (uint32_t)(c.tb - c.ta);
                    uint32_t d = kMetric == kSimPartial ? 0u : L;  // an empty Q: L insertions (partial: none)
                    if (m) {
                        if (kWide)
                            d = myers_wide<kMetric>(s_mask, s_key, m, reinterpret_cast<const uint32_t*>(M.term_bytes) + c.ta, L);
                        else d = myers_narrow<kMetric>(s_mask, m, M.term_bytes, c.ta, L);
                    }
                    sim_take<kTerms>(best, best_t, sim_of<kMetric>(d, m, L), c.tt);
                }
                if (++c.j < c.je) {
                    const uint32_t t = term_at(M, c.key, c.j);
                    c.ta = c.tb = 0;
                    if (t < M.n_terms) {
                        c.tt = t;
                        c.ta = M.term_off[t];
                        c.tb = M.term_off[t + 1];
                    }
                }
            }
            if (r < count) {
                out[r] = best;
                if constexpr (kTerms) out_t[r] = best_t;
            }
            c = nx;
        }
        return;
    }

    // ---- long path: the wave is a systolic pipeline over the query's W words ----
    const uint32_t W = (m + 63u) / 64u;
    const uint32_t rows = lane + 1u < W ? 64u : (lane < W ? m - 64u * lane : 0u);
    const uint64_t top = rows ? 1ull << (rows - 1u) : 0ull;
    const uint64_t rowmask = rows == 64u ? ~0ull : (1ull << rows) - 1ull;
    // this lane's 64 query characters: bytes packed four to a register, or one register each
    constexpr uint32_t kRegs = kWide ? 64u : 16u;
    uint32_t qw[kRegs];
#pragma unroll
    for (uint32_t i = 0; i < kRegs; ++i) qw[i] = 0;
#pragma unroll
    for (uint32_t i = 0; i < 64; ++i) {
        const uint32_t c = i < rows ? sim_norm(s_valid, ld_char(nq, 64u * lane + i, cs), cs) : 0u;
        if (kWide) qw[i] = c;
        else qw[i >> 2] |= c << (8u * (i & 3u));
    }
    for (uint32_t r = 0; r < count; ++r) {  // (the record's member is uniform over the wave)
        const uint32_t g = keys[r];
        float best = kSimNone;
        uint32_t best_t = kSimNoTerm;
        // The local key starts as the id, not as 0: a key outside the source is never read, and for one
        // index (base 0) the id is then used as loaded. Started at 0 it is a select that cost the
        // single-index kernels with terms up to 9 VGPRs and one of them a wave (profiles/sim_one_body_isa.txt).
        uint32_t j = 0, je = 0, key = g;
        const SimMember& M = src.at(g < src.total ? src.member(g) : 0u);
        if (g < src.total) {
            key = g - M.base;
            if (key < M.n_keys) key_terms(M, key, j, je);
        }
        for (; j < je; ++j) {
            const uint32_t t = term_at(M, key, j);
            if (t >= M.n_terms) continue;
            const uint64_t ta = M.term_off[t];
            const uint32_t L = (uint32_t)(M.term_off[t + 1] - ta);
            if (!L) continue;
            SimBlock<kMetric> b;
            uint32_t score = m, low = m;  // followed by lane W - 1
            int hout = 0;  // kSimOsa: the transposition bit rides in bit 2 of hout + 1
            const uint32_t steps = L + W - 1u;
            for (uint32_t s = 0; s < steps; ++s) {
                // lane w is at term character s - w, with the delta lane w - 1 left at it one step ago
                const int up = __shfl_up(hout, 1);
                int hin = lane == 0 ? kSimTopDelta<kMetric> : up;
                uint32_t tin = 0, tout = 0;
                if constexpr (kMetric == kSimOsa) {
                    tin = lane == 0 ? 0u : (uint32_t)up >> 2;
                    hin = lane == 0 ? +1 : (int)((uint32_t)up & 3u) - 1;
                }
                const uint32_t at = s - lane;
                if (lane < W && at < L) {  // (s < lane wraps past L)
                    const uint32_t c = ld_char(M.term_bytes, ta + at, cs);
                    uint64_t eq = 0;
#pragma unroll
                    for (uint32_t i = 0; i < 64; ++i) {
                        const uint32_t qi = kWide ? qw[i] : (qw[i >> 2] >> (8u * (i & 3u))) & 255u;
                        eq |= qi == c ? 1ull << i : 0ull;
                    }
                    hout = sim_step<kMetric>(b, eq & rowmask, hin, tin, top, tout);
                    if (lane == W - 1u) sim_column<kMetric>(score, low, hout);
                    if constexpr (kMetric == kSimOsa) hout = (hout + 1) | (int)(tout << 2);
                }
            }
            const uint32_t d = (uint32_t)__shfl((int)(kMetric == kSimPartial ? low : score), (int)(W - 1u));
            sim_take<kTerms>(best, best_t, sim_of<kMetric>(d, m, L), t);
        }
        if (lane == 0) {
            out[r] = best;
            if constexpr (kTerms) out_t[r] = best_t;
        }
    }
}

// Two kernels, one per source: a single index keeps its registers and its waves,
// a set pays for the member table. One wave per query, both.
template <bool kWide, uint32_t kMetric, bool kTerms>
__global__ __launch_bounds__(64) void k_sim(DevIndex X, SimArgs A) {
    const OneIndex one{{X.kt_off, X.kt_term, A.key_term, X.term_off, X.term_bytes, X.n_keys, X.n_terms, 0u, 0u}, X.n_keys};
    sim_wave<kWide, kMetric, kTerms>(one, A);
}
// The descriptors travel by value in the kernel arguments and are copied to LDS once; the members
// tile [0, total) in order (launch_similarity_set checks it).
template <bool kWide, uint32_t kMetric, bool kTerms>
__global__ __launch_bounds__(64) void k_sim_set(SimMembers T, uint32_t P, uint32_t total, SimArgs A) {
    __shared__ SimMember s_m[kSetMaxParts];
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t p = 0; p < kSetMaxParts; ++p)
            if (p < P) s_m[p] = T.m[p];  // (constant indexes: scalar loads; entries from P on are never read)
    }
    sim_wave<kWide, kMetric, kTerms>(IndexSet{s_m, P, total}, A);
}

// ---- re-rank ----
// One workgroup per query. Its size and its LDS follow the stride (launch_rerank): the sort runs over
// n2 = the count rounded up to a power of two, n2 / 2 threads (64 .. kRerankThreads) make one
// compare-exchange each per stage, and the sort keys take 8 bytes x the stride rounded up. At the
// usual limit of 100 that is one wave and 1 KiB: with a fixed 256 threads and 32 KiB, 4,096 queries of
// 100 records took 0.17 ms more.
constexpr uint32_t kRerankThreads = 256;
constexpr uint32_t kRerankPer = kRerankMaxStride / kRerankThreads;  // records a thread moves, at the most
constexpr uint32_t kRerankMinSort = 128;  // counts up to 64 take the one-wave path
__host__ __device__ inline uint32_t rerank_pow2(uint32_t n) {
    uint32_t p = kRerankMinSort;
    while (p < n) p <<= 1;
    return p;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
    return ((uint64_t)hi << 32) | lo;
}

// kTerms: a fourth array, the matched term ids, moves with the records
template <bool kTerms>
__global__ __launch_bounds__(kRerankThreads) void k_rerank(uint32_t stride, uint32_t* __restrict__ counts,
                                                            uint32_t* keys, float* scores, float* sim, float min_sim,
                                                            uint32_t* terms) {
    extern __shared__ uint64_t s_rec[];  // rerank_pow2(stride) sort keys
    __shared__ uint32_t s_kept;
    const uint32_t tid = threadIdx.x, q = blockIdx.x, nthreads = blockDim.x;
    const uint32_t count = min(counts[q], stride);
    uint32_t* k = keys + (size_t)q * stride;
    float* sc = scores + (size_t)q * stride;
    float* sv = sim + (size_t)q * stride;
    uint32_t* tv = kTerms ? terms + (size_t)q * stride : nullptr;
    if (count <= 64) {
        // one wave, no barrier: every lane holds its record, the sort runs through shuffles, and
        // a lane fetches the record of its new position from the lane that loaded it
        if (tid >= 64) return;
        const bool live = tid < count;
        const uint32_t rk = live ? k[tid] : 0u;
        const float rs = live ? sc[tid] : 0.0f, rv = live ? sv[tid] : 0.0f;
        uint32_t rt = 0;
        if constexpr (kTerms) rt = live ? tv[tid] : 0u;
        uint64_t rec = live && !(rv < min_sim) ? rerank_key(__float_as_uint(rv), tid) : kRerankDropped;
        for (uint32_t k2 = 2; k2 <= 64; k2 <<= 1)
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                const uint64_t other = shfl_xor64(rec, (int)j);
                const bool keep_min = ((tid & k2) == 0) == ((tid & j) == 0);
                rec = keep_min ? (rec < other ? rec : other) : (rec > other ? rec : other);
            }
        const uint32_t kept = (uint32_t)__popcll(__ballot(rec != kRerankDropped));
        const int src = (int)((uint32_t)rec & 63u);
        const uint32_t ok = (uint32_t)__shfl((int)rk, src);
        const float os = __shfl(rs, src), ov = __shfl(rv, src);
        uint32_t ot = 0;
        if constexpr (kTerms) ot = (uint32_t)__shfl((int)rt, src);
        if (tid < kept) {
            k[tid] = ok;
            sc[tid] = os;
            sv[tid] = ov;
            if constexpr (kTerms) tv[tid] = ot;
        }
        if (tid == 0) counts[q] = kept;
        return;
    }
    const uint32_t n2 = rerank_pow2(count);
    if (tid == 0) s_kept = 0;
    for (uint32_t i = tid; i < n2; i += nthreads) {
        uint64_t rec = kRerankDropped;
        if (i < count) {
            const float v = sv[i];
            if (!(v < min_sim)) rec = rerank_key(__float_as_uint(v), i);
        }
        s_rec[i] = rec;
    }
    __syncthreads();
    for (uint32_t k2 = 2; k2 <= n2; k2 <<= 1)
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < n2; i += nthreads) {
                const uint32_t p = i ^ j;
                if (p > i) {
                    const uint64_t a = s_rec[i], b = s_rec[p];
                    if ((a > b) == ((i & k2) == 0)) {
                        s_rec[i] = b;
                        s_rec[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    // the kept records are a prefix: its last entry reports the new count
    for (uint32_t i = tid; i < n2; i += nthreads)
        if (s_rec[i] != kRerankDropped && (i + 1 == n2 || s_rec[i + 1] == kRerankDropped)) s_kept = i + 1;
    __syncthreads();
    const uint32_t kept = s_kept;
    // in place: every record is read into registers before any is written
    uint32_t mk[kRerankPer];
    float ms[kRerankPer], mv[kRerankPer];
    uint32_t mt[kTerms ? kRerankPer : 1u];
#pragma unroll
    for (uint32_t u = 0; u < kRerankPer; ++u) {
        const uint32_t i = tid + u * nthreads;
        mk[u] = 0;
        ms[u] = mv[u] = 0.0f;
        if (i < kept) {
            const uint32_t p = (uint32_t)s_rec[i];
            mk[u] = k[p];
            ms[u] = sc[p];
            mv[u] = sv[p];
            if constexpr (kTerms) mt[u] = tv[p];
        }
    }
    // the loads of every wave have returned (s_waitcnt 0: this wave's outstanding memory operations
    // are complete; the barrier joins the waves) before any wave stores over them. A device-scope
    // fence here also wrote back and invalidated caches per workgroup: 0.10 ms per 4,096 queries.
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < kRerankPer; ++u) {
        const uint32_t i = tid + u * nthreads;
        if (i < kept) {
            k[i] = mk[u];
            sc[i] = ms[u];
            sv[i] = mv[u];
            if constexpr (kTerms) tv[i] = mt[u];
        }
    }
    if (tid == 0) counts[q] = kept;
}

// key_term[tk[p].x] = t for every pair p of term t (keys with one pair each: no two pairs write one key)
__global__ __launch_bounds__(256) void k_key_term(DevIndex X, uint32_t* __restrict__ key_term) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= X.n_terms) return;
    const uint32_t p = X.tk_identity ? t : X.tk_off[t], pe = X.tk_identity ? t + 1 : X.tk_off[t + 1];
    for (uint32_t i = p; i < pe; ++i) {
        const uint32_t key = X.tk[i].x;
        if (key < X.n_keys) key_term[key] = t;
    }
}

}  // namespace

namespace {
// The instantiation of (metric, terms, width) for either kernel: K names the kernel's family, `lead`
// are the arguments it takes in front of A. One wave per query.
struct OneIndexKernel {
    template <bool kWide, uint32_t kMetric, bool kTerms>
    static constexpr auto kernel = &k_sim<kWide, kMetric, kTerms>;
};
struct IndexSetKernel {
    template <bool kWide, uint32_t kMetric, bool kTerms>
    static constexpr auto kernel = &k_sim_set<kWide, kMetric, kTerms>;
};
template <class K, uint32_t kMetric, class... Lead>
void launch_sim_as(uint32_t cs, const SimArgs& A, hipStream_t s, const Lead&... lead) {
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(A.n), dim3(64), 0, s, lead..., A); };
    if (A.terms) go(cs == 4 ? K::template kernel<true, kMetric, true> : K::template kernel<false, kMetric, true>);
    else go(cs == 4 ? K::template kernel<true, kMetric, false> : K::template kernel<false, kMetric, false>);
}
template <class K, class... Lead>
hipError_t launch_sim(uint32_t metric, uint32_t cs, const uint32_t valid[8], SimArgs A, hipStream_t s,
                      const Lead&... lead) {
    for (int i = 0; i < 8; ++i) A.V.w[i] = valid[i];
    if (metric == kSimOsa) launch_sim_as<K, kSimOsa>(cs, A, s, lead...);
    else if (metric == kSimPartial) launch_sim_as<K, kSimPartial>(cs, A, s, lead...);
    else launch_sim_as<K, kSimLevenshtein>(cs, A, s, lead...);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_similarity(const DevIndex& X, const uint32_t valid[8], const uint32_t* key_term, const uint8_t* raw,
                             const uint64_t* off, uint32_t n, uint32_t stride, const uint32_t* counts,
                             const uint32_t* keys, uint32_t metric, float* sim, uint32_t* terms, hipStream_t s) {
    if (metric >= kSimMetrics) return hipErrorInvalidValue;
    if (!n || !stride) return hipSuccess;
    if (!X.kt_off && !key_term) return hipErrorInvalidValue;
    return launch_sim<OneIndexKernel>(metric, X.csize, valid, {raw, off, counts, keys, sim, terms, key_term, n, stride, {}},
                                      s, X);
}

hipError_t launch_similarity_set(const SimMembers& T, uint32_t P, uint32_t cs, const uint32_t valid[8],
                                 const uint8_t* raw, const uint64_t* off, uint32_t n, uint32_t stride,
                                 const uint32_t* counts, const uint32_t* keys, uint32_t metric, float* sim,
                                 uint32_t* terms, hipStream_t s) {
    if (metric >= kSimMetrics || P == 0 || P > kSetMaxParts || (cs != 1 && cs != 4)) return hipErrorInvalidValue;
    if (!n || !stride) return hipSuccess;
    uint64_t total = 0;  // the members tile [0, total) in order
    for (uint32_t p = 0; p < P; ++p) {
        const SimMember& M = T.m[p];
        if (M.base != total || (M.n_keys && !M.kt_off && !M.key_term)) return hipErrorInvalidValue;
        total += M.n_keys;
    }
    if (total > 0xFFFFFFFFull) return hipErrorInvalidValue;
    return launch_sim<IndexSetKernel>(metric, cs, valid, {raw, off, counts, keys, sim, terms, nullptr, n, stride, {}}, s, T,
                                      P, (uint32_t)total);
}

hipError_t launch_rerank(uint32_t n, uint32_t stride, uint32_t* counts, uint32_t* keys, float* scores, float* sim,
                         uint32_t* terms, float min_sim, hipStream_t s) {
    if (!n) return hipSuccess;
    if (stride > kRerankMaxStride) return hipErrorInvalidValue;
    const uint32_t n2 = rerank_pow2(stride);  // every count's sort fits: counts are read as at most the stride
    const uint32_t threads = n2 / 2 < 64 ? 64 : (n2 / 2 > kRerankThreads ? kRerankThreads : n2 / 2);
    static_assert(kRerankPer * kRerankThreads == kRerankMaxStride, "a thread moves at most kRerankPer records");
    if (terms)
        hipLaunchKernelGGL(k_rerank<true>, dim3(n), dim3(threads), sizeof(uint64_t) * n2, s, stride, counts, keys, scores,
                           sim, min_sim, terms);
    else
        hipLaunchKernelGGL(k_rerank<false>, dim3(n), dim3(threads), sizeof(uint64_t) * n2, s, stride, counts, keys, scores,
                           sim, min_sim, terms);
    return hipGetLastError();
}

hipError_t build_key_term(const DevIndex& X, uint32_t* key_term, hipStream_t s) {
    hipError_t e = hipMemsetAsync(key_term, 0xFF, sizeof(uint32_t) * (size_t)(X.n_keys ? X.n_keys : 1u), s);
    if (e != hipSuccess || !X.n_terms) return e;
    hipLaunchKernelGGL(k_key_term, dim3((X.n_terms + 255u) / 256u), dim3(256), 0, s, X, key_term);
    return hipGetLastError();
}

}  // namespace ngs
