// Host model of the main tier-1a launch's planner (lean_query_g) for tests/test_lean_plan_model.py,
// built with g++ alone from ngs_common.h: the lane apportionment (group_share, group_rem_key,
// group_quota, called as the kernel calls them) over random length vectors, and a restatement of the
// greedy part cut (part_entry_limit, steps of 2^ush buckets, the sub-part path as term-id ranges) over
// random sorted lists and their skip tables. Prints one line per check group; exit status 1 on a miss.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "ngs_common.h"

using namespace ngs;

static int g_fail = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            if (++g_fail <= 20) {              \
                std::printf("FAIL %s: ", #c);  \
                std::printf(__VA_ARGS__);      \
                std::printf("\n");             \
            }                                  \
        }                                      \
    } while (0)

// the kernel's set-up: lane j < ng holds list j's share; the lanes left over after the floors
static std::vector<uint32_t> quotas(const std::vector<uint32_t>& len) {
    const uint32_t ng = (uint32_t)len.size();
    uint64_t P = 0;
    for (uint32_t l : len) P += l;
    std::vector<uint64_t> share(ng);
    std::vector<uint32_t> key(ng), q(ng);
    uint32_t floors = 0;
    for (uint32_t j = 0; j < ng; ++j) {
        share[j] = group_share(ng, len[j], P);
        key[j] = group_rem_key(share[j], j);
        floors += (uint32_t)(share[j] >> kShareBits);
    }
    const uint32_t left = 64u - ng - floors;
    for (uint32_t j = 0; j < ng; ++j) q[j] = group_quota(ng, j, share[j], left, [&](uint32_t k) { return key[k]; });
    return q;
}

static void check_quota(const std::vector<uint32_t>& len, const char* what) {
    const uint32_t ng = (uint32_t)len.size();
    const std::vector<uint32_t> q = quotas(len);
    uint64_t P = 0;
    for (uint32_t l : len) P += l;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < ng; ++j) {
        CHECK(q[j] >= 1, "%s ng=%u list %u has no lane", what, ng, j);
        sum += q[j];
        // len / quota <= 2 * (P / 64), in integers
        if (ng <= 32) CHECK((uint64_t)len[j] * 64u <= 2u * P * q[j], "%s ng=%u len=%u quota=%u P=%llu", what, ng, len[j], q[j], (unsigned long long)P);
    }
    CHECK(sum == 64, "%s ng=%u quotas sum to %u", what, ng, sum);
    // largest remainder: with the exact shares s_j, every quota is floor(1 + s_j) or that plus one
    for (uint32_t j = 0; j < ng; ++j) {
        const uint64_t fl = 1u + ((uint64_t)(64u - ng) * len[j]) / P;
        CHECK(q[j] == fl || q[j] == fl + 1, "%s ng=%u quota %u floor %llu", what, ng, q[j], (unsigned long long)fl);
    }
}

static uint32_t chunks(uint32_t a0, uint32_t s, uint32_t e) { return e > s ? ((a0 + e + 3) >> 2) - ((a0 + s) >> 2) : 0u; }

struct Part {
    uint32_t lo, hi;  // term ids [lo, hi)
    bool fast;
};

// the greedy cut over lists of sorted term ids; returns the parts and checks each as it is made
static void check_cut(std::mt19937_64& rng, uint32_t ng, uint32_t n_long, uint32_t K, double dense, uint32_t hot, bool shrink2) {
    const uint32_t span = (n_long + K - 1) / K;
    std::vector<std::vector<uint32_t>> list(ng);
    std::vector<uint32_t> len(ng), a0(ng);
    const uint32_t t_lo = rng() % 3 == 0 ? n_long / 4 : 0, t_hi = rng() % 3 == 0 ? n_long - n_long / 3 : n_long;  // empty ends
    for (uint32_t j = 0; j < ng; ++j) {
        const double p = j < hot ? 0.3 : dense * (0.25 + (double)(rng() % 1000) / 500.0);
        std::bernoulli_distribution coin(std::min(p, 1.0));
        for (uint32_t t = t_lo; t < t_hi; ++t)
            if (coin(rng)) list[j].push_back(t);
        if (list[j].empty()) list[j].push_back(t_lo + (uint32_t)(rng() % (t_hi - t_lo)));
        len[j] = (uint32_t)list[j].size();
        a0[j] = (uint32_t)(rng() & 3u);
    }
    std::vector<std::vector<uint32_t>> skip(ng, std::vector<uint32_t>(K + 1));
    for (uint32_t j = 0; j < ng; ++j)
        for (uint32_t b = 0; b <= K; ++b)
            skip[j][b] = (uint32_t)(std::lower_bound(list[j].begin(), list[j].end(), (uint64_t)b * span > n_long ? n_long : b * span) - list[j].begin());
    uint64_t P = 0;
    for (uint32_t l : len) P += l;
    const std::vector<uint32_t> G = quotas(len);
    std::vector<uint32_t> capc(ng), cur(ng, 0);
    uint32_t gmin = 64;
    for (uint32_t j = 0; j < ng; ++j) {
        capc[j] = std::min(3u * G[j], std::max(2u, (3u * G[j]) >> (shrink2 ? kLeanShrink2 : 0u)));
        gmin = std::min(gmin, G[j]);
    }
    const uint32_t target = (uint32_t)kGroupTarget >> (shrink2 ? kLeanShrink2 : 0u);
    const uint32_t wspan = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(K, kMaxPartSpan / std::max(span, 1u)));
    const uint32_t wmax = std::min(std::min(gmin, kMaxPartWidth), wspan);
    const uint32_t ush = part_step_shift(wmax, wspan, (uint64_t)K * target / P);
    CHECK((wmax << ush) <= wspan, "widest part %u buckets of %u", wmax << ush, wspan);
    std::vector<Part> parts;
    std::vector<uint64_t> in_parts(ng, 0);
    auto take = [&](uint32_t lo, uint32_t hi, const std::vector<uint32_t>& e, bool fast) {
        bool any = false;
        for (uint32_t j = 0; j < ng; ++j) {
            for (uint32_t i = cur[j]; i < e[j]; ++i) CHECK(list[j][i] >= lo && list[j][i] < hi, "posting %u of list %u outside [%u, %u)", list[j][i], j, lo, hi);
            if (e[j] < len[j]) CHECK(list[j][e[j]] >= hi, "list %u: posting %u left behind by part [%u, %u)", j, list[j][e[j]], lo, hi);
            const uint32_t nch = chunks(a0[j], cur[j], e[j]);
            if (fast) CHECK(nch <= capc[j], "fast part [%u, %u): list %u has %u chunks, cap %u", lo, hi, j, nch, capc[j]);
            if (hi - lo > 1) CHECK(nch <= capc[j], "sub-part [%u, %u): list %u has %u chunks, cap %u", lo, hi, j, nch, capc[j]);
            // the limit the kernel compares against is the chunk rule
            CHECK((nch <= capc[j]) == (e[j] <= part_entry_limit(a0[j], cur[j], capc[j])), "entry limit: a0 %u cur %u e %u cap %u", a0[j], cur[j], e[j], capc[j]);
            any = any || e[j] > cur[j];
            in_parts[j] += e[j] - cur[j];
            cur[j] = e[j];
        }
        CHECK(parts.empty() ? lo == 0 : parts.back().hi == lo, "part [%u, %u) does not follow the last", lo, hi);
        parts.push_back({lo, hi, fast});
        (void)any;  // (the kernel skips a part whose segments are all empty; the tiling is the same)
    };
    uint32_t b = 0;
    std::vector<uint32_t> e(ng);
    while (b < K) {
        uint32_t t = 0;
        while (t < wmax) {  // monotone: the first step count that fails ends the search
            bool fits = true;
            for (uint32_t j = 0; j < ng; ++j)
                fits = fits && skip[j][std::min(K, b + ((t + 1) << ush))] <= part_entry_limit(a0[j], cur[j], capc[j]);
            if (!fits) break;
            ++t;
        }
        if (t) {
            const uint32_t bhi = std::min(K, b + (t << ush));
            for (uint32_t j = 0; j < ng; ++j) e[j] = skip[j][bhi];
            if (t < wmax && bhi < K) {  // greedy: one more step would have put some list over its cap
                bool over = false;
                for (uint32_t j = 0; j < ng; ++j)
                    over = over || chunks(a0[j], cur[j], skip[j][std::min(K, b + ((t + 1) << ush))]) > capc[j];
                CHECK(over, "part at bucket %u stops at %u steps although %u fit", b, t, t + 1);
            }
            take(b * span, (uint32_t)std::min<uint64_t>((uint64_t)bhi * span, n_long), e, true);
            b = bhi;
            continue;
        }
        // one step over a cap: term-id sub-ranges, halved until every list fits or one term is left
        const uint32_t bhi = std::min(K, b + (1u << ush));
        uint32_t lo = b * span;
        const uint32_t hi_lim = (uint32_t)std::min<uint64_t>((uint64_t)bhi * span, n_long);
        uint32_t step = hi_lim - lo;
        while (lo < hi_lim) {
            const uint32_t hi = (uint32_t)std::min<uint64_t>(hi_lim, (uint64_t)lo + step);
            bool fits = true;
            for (uint32_t j = 0; j < ng; ++j) {
                e[j] = (uint32_t)(std::lower_bound(list[j].begin() + cur[j], list[j].begin() + skip[j][bhi], hi) - list[j].begin());
                fits = fits && chunks(a0[j], cur[j], e[j]) <= capc[j];
            }
            if (!fits && hi - lo > 1) {
                step = std::max(1u, (hi - lo) / 2);
                continue;
            }
            take(lo, hi, e, false);
            lo = hi;
        }
        b = bhi;
    }
    CHECK(!parts.empty() && parts.front().lo == 0 && parts.back().hi >= std::min<uint64_t>((uint64_t)K * span, n_long), "parts end at %u of %u", parts.empty() ? 0u : parts.back().hi, n_long);
    for (uint32_t j = 0; j < ng; ++j) CHECK(in_parts[j] == len[j] && cur[j] == len[j], "list %u: %llu of %u postings in parts", j, (unsigned long long)in_parts[j], len[j]);
}

int main() {
    std::mt19937_64 rng(20240607);
    // ---- quotas ----
    int n = 0;
    for (int it = 0; it < 4000; ++it, ++n) {
        const uint32_t ng = 1u + (uint32_t)(rng() % 64);
        std::vector<uint32_t> len(ng);
        const uint32_t top = 1u << (rng() % 21);  // lengths 1 .. 10^6, every magnitude
        for (auto& l : len) l = 1u + (uint32_t)(rng() % std::min<uint64_t>(1000000, top));
        check_quota(len, "random");
    }
    for (uint32_t ng = 2; ng <= 64; ++ng, ++n) {  // one list with 99 % of the postings
        std::vector<uint32_t> len(ng, 1u + (uint32_t)(rng() % 100));
        uint64_t rest = 0;
        for (uint32_t j = 1; j < ng; ++j) rest += len[j];
        len[rng() % ng] = (uint32_t)std::min<uint64_t>(1000000, 99 * rest);
        check_quota(len, "99 %");
    }
    for (uint32_t ng = 1; ng <= 64; ++ng)
        for (uint32_t l : {1u, 7u, 4096u, 1000000u}) {
            check_quota(std::vector<uint32_t>(ng, l), "equal");
            ++n;
        }
    for (uint32_t ng : {63u, 64u})
        for (int it = 0; it < 200; ++it, ++n) {
            std::vector<uint32_t> len(ng);
            for (auto& l : len) l = 1u + (uint32_t)(rng() % 1000000);
            check_quota(len, "63/64");
        }
    std::printf("quota vectors checked: %d\n", n);
    // ---- the cut ----
    int m = 0;
    for (int it = 0; it < 300; ++it, ++m) {
        const uint32_t ng = 1u + (uint32_t)(rng() % (it % 5 == 0 ? 63 : 14));
        const uint32_t K = 1u << (2 + rng() % 4);  // 4 .. 32 buckets
        const uint32_t n_long = K * (40 + (uint32_t)(rng() % 400)) - (uint32_t)(rng() % 7);
        const double dense = it % 7 == 0 ? 0.002 : 0.01 + 0.12 * (double)(rng() % 100) / 100.0;
        check_cut(rng, ng, n_long, K, dense, it % 4 == 0 ? 2u : 0u, it % 6 == 0);
    }
    std::printf("cuts checked: %d\n", m);
    std::printf(g_fail ? "FAILED: %d\n" : "ok\n", g_fail);
    return g_fail ? 1 : 0;
}
