"""Planted libraries and queries for tier 2 (k_fast / fast_one, ngs_kernels.hip), and the CPU facts
about them. tests/test_fast_cases.py proves every claim on the CPU; tests/test_gpu_fast_planted.py
runs the libraries on the device and asserts that the index reports the geometry recorded here.

What fast_one does with a query, restated from the rows alone (plan):
  ng        its distinct grams that have a list;
  p_total   those lists' lengths, each distinct gram once;
  btot[b]   the postings of those lists in term-id bucket b. The planner sees at most kMaxBuckets
            (256) buckets: an index with more (dense lists, skip_buckets in ngs_common.h) is read at
            every kst-th boundary, so its planner buckets are kst index buckets wide;
  class     "one"   p_total <= kPartCap (4,096): one part, base 0;
            "over"  some btot[b] > kPartCap: that bucket is cut into term-id sub-parts;
            "multi" otherwise, when the greedy cut of the bucket sequence into whole-bucket parts of
                    <= kPartCap postings gives at least 3 parts ("two" when it gives 2);
  switches  how often the sequence of non-empty buckets changes between oversized and whole.

The skip table's geometry follows from the lists: K doubles from 16 (40,000 terms) while the longest
list has more than 16 postings per bucket. A list long enough to put three grams' postings above
4,096 in one bucket of 2,500 ids would push K to 1,024 and the planner's buckets down to about 160
ids, which 10..15-letter rows cannot fill with 4,096 postings. So library P keeps every list under
1,088 postings (K = 64, span = 625, kst = 1) and plants hot STRINGS of 12 letters (10 grams) instead
of single hot grams: in its hot bucket a hot string is in about 79 % of the rows, so each of its ten
lists has about 490 postings there and the ten together about 4,900.

The libraries:
  P  planner: 39,994 distinct rows of 10..15 letters, A..M with a band over N..Z in the middle, three
     hot strings (hot in buckets 1, 3 and 5, rare elsewhere), six rows of 257 characters at the end
     (255 distinct grams; one gram 255 times; two grams 128 + 127 times; a one-character variant of
     each), and a second exact-table chain planted relative to the second part of a "multi" query;
  T  table chain: 40,000 rows, fillers over the letters, 33 planted terms over the digits and . % $ @
     whose relative ids (id + 1: one part, base 0) home into the slots 8185..8191 and 0..10;
  D  buffer and dedup: 12,300 rows of a key and two aliases, one hot gram in most alias terms;
  W  P's short rows as a wide index of gram size 2.
"""
import os
import random
import re

import hash_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON_H = os.path.join(ROOT, "stringsearchlib_amd", "csrc", "ngs_common.h")


def _constant(name, text):
    m = re.search(rf"constexpr \w+ {name} = (\d+);", text)
    if not m:
        raise RuntimeError(f"fast_cases: {name} not found in {COMMON_H}: tier 2's geometry moved, so the planted "
                           f"inputs of tests/fast_cases.py must be looked at again")
    return int(m.group(1))


def read_geometry(text=None):
    if text is None:
        with open(COMMON_H) as f:
            text = f.read()
    return {k: _constant(k, text) for k in ("kTableSlots", "kCandCap", "kFastMaxGrams", "kMaxBuckets")}


GEOM = read_geometry()
SLOTS, CAND_CAP, MAX_GRAMS, MAX_BUCKETS = GEOM["kTableSlots"], GEOM["kCandCap"], GEOM["kFastMaxGrams"], GEOM["kMaxBuckets"]
SLOT_BITS = SLOTS.bit_length() - 1
PART_CAP = SLOTS // 2  # kPartCap
if SLOTS != 1 << 13 or CAND_CAP != 2048 or MAX_GRAMS != 255:
    raise RuntimeError("fast_cases: the planted homes, counts and buffer fills are for 8,192 slots, 2,048 records and "
                       "255 grams")

# The skip-table geometry (K, span) the device build reported for each library (ngsIndexDigest words 2
# and 7). The GPU test asserts that the digest still reports these.
P_GEOM = (64, 625)
W_GEOM = (256, 156)
D_GEOM = (1024, 37)

AM, NZ = "ABCDEFGHIJKLM", "NOPQRSTUVWXYZ"
LETTERS = AM + NZ
PLANT = "0123456789.%$@"


def grams(s, g=3):
    """The grams of a string in order, with repeats."""
    return [s[i:i + g] for i in range(len(s) - g + 1)]


def lists_of(terms, g=3):
    """{gram: ascending long-term ids} of a library whose every term is long and whose term id is its
    position in `terms`."""
    out = {}
    for i, t in enumerate(terms):
        for x in set(grams(t, g)):
            out.setdefault(x, []).append(i)
    return out


def check_geometry(n_long, K, span):
    """The planner reads the index's own buckets (kst = 1), and they cover the terms exactly."""
    assert (K - 1) * span < n_long <= K * span, (n_long, K, span)
    assert K <= MAX_BUCKETS, K


def planner_buckets(K, span):
    kst = K // MAX_BUCKETS if K > MAX_BUCKETS else 1
    return K // kst, span * kst


class Plan:
    pass


def plan(lists, query, K, span, g=3):
    """fast_one's view of `query` on a library with the lists `lists` and the skip geometry (K, span)."""
    p = Plan()
    distinct = list(dict.fromkeys(grams(query, g)))
    have = [lists[x] for x in distinct if lists.get(x)]
    kp, sp = planner_buckets(K, span)
    p.ng = len(have)
    p.p_total = sum(map(len, have))
    p.btot = [0] * kp
    for ids in have:
        for i in ids:
            p.btot[i // sp] += 1
    p.span = sp
    p.parts = []  # (first bucket, end bucket, oversized)
    if p.p_total <= PART_CAP:
        if p.p_total:
            p.parts.append((0, kp, False))
        p.cls = "one"
    else:
        b = 0
        while b < kp:
            if p.btot[b] > PART_CAP:
                p.parts.append((b, b + 1, True))
                b += 1
                continue
            lo, tot = b, 0
            while b < kp and tot + p.btot[b] <= PART_CAP:
                tot += p.btot[b]
                b += 1
            if tot:
                p.parts.append((lo, b, False))
        if any(o for _, _, o in p.parts):
            p.cls = "over"
        else:
            p.cls = "multi" if len(p.parts) >= 3 else "two"
    kinds = [t > PART_CAP for t in p.btot if t]
    p.switches = sum(a != b for a, b in zip(kinds, kinds[1:]))
    return p


# ---- planted terms ---------------------------------------------------------------------------
class Planter:
    """Terms that share an exact number of distinct grams with a query of unrepeated grams: a run of the
    query with a pad over the digits and . % $ @ before or behind it."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.terms = set()

    def query(self, length):
        while True:
            q = "".join(self.rng.choices(PLANT, k=length))
            if len(set(grams(q))) == length - 2:
                return q

    def term(self, q, hits):
        own = set(grams(q))
        while True:
            s = self.rng.randrange(len(q) - hits - 1)
            body = q[s:s + hits + 2]
            pad = "".join(self.rng.choices(PLANT, k=max(0, 6 - len(body)) + self.rng.randint(1, 3)))
            t = body + pad if self.rng.random() < 0.5 else pad + body
            if len(set(grams(t)) & own) == hits and t not in self.terms:
                self.terms.add(t)
                return t


def homing(lo_slot, hi_slot, n_rel):
    """The relative ids 1..n_rel whose home slot in tier 2's table is in lo_slot..hi_slot."""
    return [r for r in range(1, n_rel + 1) if lo_slot <= hc.exact_home(r, SLOT_BITS) <= hi_slot]


# ---- library P ---------------------------------------------------------------------------------
P_ROWS, P_LONG_ROWS = 40000, 6
P_BASE = P_ROWS - P_LONG_ROWS
P_BAND = (15000, 25000)       # the rows over N..Z
P_HOT_BUCKETS = (1, 3, 5)     # hot string j is hot in bucket P_HOT_BUCKETS[j]
P_LOW = 0.01                  # and this likely in every other A..M row
P_THRESHOLDS = (0.0, 0.3, 1.0)


def hot_strings():
    """Three strings of 12 different letters of A..M with 30 different grams between them."""
    rng = random.Random(41)
    out, seen = [], set()
    while len(out) < 3:
        h = "".join(rng.sample(AM, 12))
        if not seen & set(grams(h)):
            seen |= set(grams(h))
            out.append(h)
    return out


def long_rows():
    """R1 (255 distinct grams), R2 (one gram 255 times), R3 (two grams, 128 and 127 times), then a
    variant of each with the character in the middle changed."""
    rng = random.Random(43)
    r1, used = "AB", set()
    while len(r1) < 257:
        c = next(c for c in rng.sample(AM, len(AM)) if r1[-2:] + c not in used)
        used.add(r1[-2:] + c)
        r1 += c
    r2, r3 = "A" * 257, "AB" * 128 + "A"
    vary = {r1: next(c for c in AM if c not in r1[126:131]), r2: "B", r3: "C"}
    return [r1, r2, r3] + [r[:128] + vary[r] + r[129:] for r in (r1, r2, r3)]


def _p_base_rows(span):
    hot = hot_strings()
    p_hot = 1.2 * PART_CAP / (10 * span)  # ten lists of span * p_hot postings: 20 % over the cap
    assert p_hot <= 0.9, "the hot bucket cannot hold the cap: the geometry moved"
    rng = random.Random(79)
    seen, rows = set(), []
    for i in range(P_BASE):
        letters = NZ if P_BAND[0] <= i < P_BAND[1] else AM
        h = None
        if letters is AM:
            h = next((h for j, h in enumerate(hot)
                      if rng.random() < (p_hot if i // span == P_HOT_BUCKETS[j] else P_LOW)), None)
        while True:
            w = "".join(rng.choices(letters, k=rng.randint(10, 15)))
            if h:  # 14 or 15 letters: enough different rows around one string
                w = "".join(rng.choices(AM, k=rng.randint(14, 15)))
                at = rng.randrange(len(w) - 11)
                w = w[:at] + h + w[at + 12:]
            if w not in seen:
                break
        seen.add(w)
        rows.append(w)
    return rows


def _chain_of(rows, n):
    """n characters of rows laid end to end."""
    return "".join(rows)[:n]


class LibP:
    def __init__(self, geom=P_GEOM):
        self.K, self.span = geom
        self.hot = hot_strings()
        rows = _p_base_rows(self.span) + long_rows()
        self.n_long = len(rows)
        rng = random.Random(5)
        am = [r for i, r in enumerate(rows[:P_BASE]) if not P_BAND[0] <= i < P_BAND[1] and not any(h in r for h in self.hot)]
        nz = rows[P_BAND[0]:P_BAND[1]]

        def cut(pool, n):
            """n characters cut from rows of the pool laid end to end, one of them changed."""
            w = _chain_of(rng.sample(pool, n // 10 + 2), n + 8)
            s = rng.randrange(8)
            w = list(w[s:s + n])
            w[rng.randrange(n)] = rng.choice(NZ if pool is nz else AM)
            return "".join(w)

        # the second exact-table chain: relative to the second part of this query (a "multi" one)
        base_lists = lists_of(rows)
        cands = [cut(am, n) for n in (80, 90, 100, 110, 120) for _ in range(4)]
        cands = [q for q in cands if len(set(grams(q))) == len(q) - 2]
        best = None
        for q in cands:
            pl = plan(base_lists, q, self.K, self.span)
            if pl.cls == "multi":
                lo, hi = pl.parts[1][0] * pl.span, min(pl.parts[1][1] * pl.span, P_BASE)
                rs = [r for r in homing(SLOTS - 4, SLOTS - 1, hi - lo)]
                if best is None or len(rs) > len(best[1]):
                    best = (q, rs, lo)
        self.chain_query, self.chain_rels, self.chain_lo = best
        planter = Planter(47)
        self.chain_plan = {}  # term id -> (term, hits)
        for k, r in enumerate(self.chain_rels):
            i = self.chain_lo + r - 1
            rows[i] = planter.term(self.chain_query, 3 + k)
            self.chain_plan[i] = (rows[i], 3 + k)
        assert len(set(rows)) == len(rows)
        self.rows = rows
        self.lists = lists_of(rows)

        h0, h1, h2 = self.hot
        filler = _chain_of(rng.sample(am, 16), 140)
        self.queries = {
            "one": [cut(am, 12) for _ in range(6)] + [cut(am, 9), cut(am, 16)],
            "band": [cut(nz, 12), cut(nz, 12), cut(nz, 70)],
            "multi": [self.chain_query] + [cut(am, n) for n in (75, 85, 95, 105, 120)],
            "over": [h0, h1, h2, "K" + h1, h2 + "AC", h0 + h2, h0 + h1 + h2, filler[:64] + h1 + filler[76:]],
        }
        r = rows[P_BASE:]
        self.long_queries = list(r)
        self.controls = [r[0] + next(c for c in AM if r[0][-2:] + c not in set(grams(r[0]))), r[1] + "A", r[2] + "B"]
        self.plans = {q: plan(self.lists, q, self.K, self.span) for q in self.all_queries() + self.long_queries}

    def all_queries(self):
        return [q for kind in ("one", "band", "multi", "over") for q in self.queries[kind]]


# ---- library T ---------------------------------------------------------------------------------
T_ROWS = 40000
T_THRESHOLDS = (0.0, 0.3, 0.6)
T_LIMIT = 129


class LibT:
    def __init__(self):
        planter = Planter(53)
        self.query = planter.query(40)
        self.tail = [r - 1 for r in homing(SLOTS - 4, SLOTS - 1, T_ROWS)]   # every such id: the chain
        used = set(self.tail)

        def first_homing(slot):
            i = next(r - 1 for r in homing(slot, slot, T_ROWS) if r - 1 not in used)
            used.add(i)
            return i

        self.displaced = [first_homing(s) for s in range(11)]            # slots 0..10
        self.lead = [first_homing(s) for s in (SLOTS - 7, SLOTS - 6, SLOTS - 5)]
        ids = self.tail + self.displaced + self.lead
        hits = list(range(3, 3 + len(ids)))
        random.Random(59).shuffle(hits)
        self.plan = {i: (planter.term(self.query, h), h) for i, h in zip(ids, hits)}
        rng = random.Random(61)
        seen, rows = set(), []
        for i in range(T_ROWS):
            if i in self.plan:
                rows.append(self.plan[i][0])
                continue
            while True:
                w = "".join(rng.choices(LETTERS, k=rng.randint(8, 12)))
                if w not in seen:
                    break
            seen.add(w)
            rows.append(w)
        self.rows = rows
        self.lists = lists_of(rows)


# ---- library D ---------------------------------------------------------------------------------
D_KEYS = 12300
D_HOT = "QZX"
D_P_HOT = 0.6
D_THRESHOLDS = (0.0, 0.2)
D_LIMITS = (129, 1024)
# (weight of the first alias, of the second) by key number mod 10
D_WEIGHTS = [(1.0, 2.0), (0.5, 1.75), (1.25, 1.5), (2.0, 1.0), (1.75, 0.5), (1.5, 1.25), (1.5, 1.5), (0.75, 0.75),
             (-1.0, 1.25), (1.25, -0.5)]


class LibD:
    """Rows of a key and two aliases, every word a term of its own (8..12 letters over A..P, distinct),
    so a word's term id is its position. The hot gram QZX is written into 60 % of the aliases."""

    def __init__(self):
        rng = random.Random(67)
        seen, words, wts = set(), [], []
        for k in range(D_KEYS):
            for j in range(3):
                while True:
                    w = "".join(rng.choices(LETTERS[:16], k=rng.randint(8, 12)))
                    if j and rng.random() < D_P_HOT:
                        at = rng.randrange(len(w) - 2)
                        w = w[:at] + D_HOT + w[at + 3:]
                    if w not in seen:
                        break
                seen.add(w)
                words.append(w)
                wts.append(1.0 if j == 0 else D_WEIGHTS[k % 10][j - 1])
        self.words, self.weights = words, wts
        self.lists = lists_of(words)
        aliases = [w for i, w in enumerate(words) if i % 3]
        self.queries = []
        for n in range(18):
            a = rng.choice(aliases).replace(D_HOT, "")
            at = rng.randrange(0, 7)
            self.queries.append((a[:at] + D_HOT + a[at:] + "ABCDEFGHIJKL")[:12])


# ---- library W ---------------------------------------------------------------------------------
W_ROWS = 39936  # 256 * 156: a whole number of buckets at K = 256


def w_rows(p):
    """P's rows without the 257-character ones (and without the few beyond 256 whole buckets)."""
    return p.rows[:W_ROWS]


def d_pairs(lib, model):
    """{term id: (key rank, weight)} from the build model (build_ref.build): in D every term has one pair."""
    import build_ref
    assert len(model.terms) == len(lib.words) and model.n_short == 0
    assert all(len(p) == 1 for p in model.tk)
    return {t: (p[0][0], build_ref.bits_f32(p[0][1])) for t, p in enumerate(model.tk)}


def d_facts(lib, pairs, query, bucket_span):
    """What a threshold-0 search of `query` scores in D: the number of scored terms, and among the keys
    both of whose alias terms are scored how many have their best w * s (fp32, as calcScore) on the
    alias with the larger term id, on the smaller, on both alike (equal bits), how many have a
    negative weight beside a positive one, and how many have the two aliases in different buckets."""
    import numpy as np
    n = np.float32(len(query) - 2)
    count = {}
    mult = {}
    for x in grams(query):
        mult[x] = mult.get(x, 0) + 1
    for x, k in mult.items():
        for t in lib.lists.get(x, ()):
            count[t] = count.get(t, 0) + k
    by_key = {}
    for t in count:
        if t % 3:  # an alias: words 3k + 1 and 3k + 2
            by_key.setdefault(pairs[t][0], []).append(t)
    out = {"terms": len(count), "both": 0, "larger": 0, "smaller": 0, "equal": 0, "negative": 0, "split": 0}
    for ts in by_key.values():
        if len(ts) != 2:
            continue
        a, b = sorted(ts)
        va, vb = (max(np.float32(pairs[t][1]) * (np.float32(count[t]) / n), np.float32(0)) for t in (a, b))
        out["both"] += 1
        out["larger"] += bool(vb > va)
        out["smaller"] += bool(va > vb)
        out["equal"] += bool(va == vb)
        out["negative"] += min(pairs[a][1], pairs[b][1]) < 0 < max(pairs[a][1], pairs[b][1])
        out["split"] += a // bucket_span != b // bucket_span
    return out


def w_queries(p):
    return (["ABC", "NOP", "MLK", "ABCD"] + p.queries["one"][:5] + p.queries["band"] + p.queries["multi"][:2]
            + p.queries["over"][:3] + p.queries["over"][-2:])
