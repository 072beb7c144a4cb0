"""Planted collisions in the search path's hash structures, exact against the oracle.

Count sketch (ngs_kernels.hip: sketch_cell, part_sketch / lean_sketch_g, part_ones, cand_counts):
narrow libraries at gram size 3 whose keys are their own long terms, so a long-term id is a
position in the word list. Fillers are strings over the letters; the planted terms and the queries
are over the digits and . % $ @ only, every group of planted terms has a query of its own, and no
planted term shares a gram with another group's query (asserted below), so a query's lists hold its
group's terms and nothing else. A handful of postings is far below every part target, so the
planner's bucket group is the whole skip table (w = K in lean_query, lean_query_g and wave_query) and
the group's terms, whole tables of ids apart, are counted in one part, in one cell
(tests/test_hash_cases.py).

Tier 1a (cells: the id's low 13 bits; ids 8,192 apart), one 40-character query (38 grams) per group,
in batches of 17 (up to 16 queries take the latency path), at thresholds that put cmin below,
between and above the hit counts:
  a (6, 5)          both pass, or one, or none although the cell holds 11
  b (9, 3)          the 9 alone survives, with count 9 and not 12
  c (4, 4)          neither passes cmin 5..8 although the cell holds 8
  d (8, 7)          the cell holds 15: full, not wrapped
  e (8, 8)          16 and more: the counter wraps; the wrap is seen on the returning add and the
                    query is handed over to exact counting (handover_queries)
  f (16, 3) + 5     a term that wraps alone, a partner, and 5 hits in the next cell (id + 1), which
                    receives the carry
  g as f, cell % 8 == 7: the carry leaves the word
  h (5, 4, 3)       three terms in one cell
  ones: (1, 1), (1, 4) and twelve pairs of (3, 3) against 20-character queries at threshold 0: on the
  weighted library part_ones (two one-hit terms in a cell, a one-hit beside a multi-hit term, and 72
  entries in shared cells, more than the 64 a part resolves: handed over); on the one-weight library
  the rank lists take threshold 0 at cmin 2.
The sketch's add pass also counts the up to 3 ids of neighbouring lists in the 16-byte chunks at each
end of a list (never an undercount), and here those are planted terms too. sketch_view models that
on the CPU; the planter's seed is one for which the strays take no group past 15 that is not meant
to wrap, and leave d at exactly 15 (e's cell sees 19).
Routes asserted with last_stats(): cmin >= 3 finishes in the main tier-1a launch (no heavy, full or
tier-2 query; handed over exactly when a counter wraps), cmin <= 2 goes to the heavy list.

Full kernel (cells: id ^ id >> 14): what the part can reach. A batch's full list and hand-overs run
as four term-id slices, one wave each, so in a library of this size no two ids of one wave share a
cell; an unsliced wave needs the latency path (up to 16 queries) on a library of one group of 8
skip buckets, at most 32,768 long terms, where every cell has exactly two ids, x and
16384 + (x ^ 1). So the full-kernel groups are pairs on 32,768 long terms through batches of 3, with
sums of 11, 8, 16 and 19; three terms of 6 hits on the short-search route cannot share a cell. The
full kernel falls back to exact counting inside the wave, which no counter shows.

Exact table (wave_insert_slot, the full kernel at cmin 1): on the same path a part's base is 0, so
a term's relative id is id + 1 and its home slot (rel * 0x9E3779B1) >> 21 can be planted: twelve
terms homing into the last 4 of 2,048 slots, a chain that wraps. Tier 2's table_insert takes its
base from k_fast's own part planner, which cuts by the postings of the whole query; it is planted in
tests/test_gpu_fast_planted.py (tests/fast_cases.py: base 0 and the base of a second part).

Gram dictionary (gram_at's open addressing, set_gram_dict): wide indexes whose every gram homes
into the last slots of the table, so the one chain wraps to slot 0; queries mix present grams with
absent ones that home into the chain (the lookup walks it, wraps and stops at the first empty slot)
and absent ones that home onto an empty slot. tests/hash_cases.py plants the code points and
tests/test_hash_cases.py proves the layout on the CPU.
"""
import random
import struct

import pytest
import torch

import hash_cases as hc
import stringsearchlib_amd as ssl
from oracle_py import OracleIndexG
from test_gpu_parity import assert_exact

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _device_answers(gi, queries, thr, limit):
    """search_device over UTF-32 query bytes; ids mapped to keys with key()."""
    units = [[ord(c) for c in q] for q in queries]
    flat = b"".join(struct.pack(f"<{len(u)}I", *u) for u in units)
    offs = [0]
    for u in units:
        offs.append(offs[-1] + 4 * len(u))
    raw = torch.frombuffer(bytearray(flat) or bytearray(4), dtype=torch.uint8).to(DEV)
    off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    stride = max(1, min(limit, gi.num_keys()))
    counts = torch.zeros(len(queries), dtype=torch.int32, device=DEV)
    keys = torch.zeros(len(queries) * stride, dtype=torch.int32, device=DEV)
    scores = torch.zeros(len(queries) * stride, dtype=torch.float32, device=DEV)
    gi.search_device(raw.data_ptr(), off.data_ptr(), len(queries), thr, limit, stride, counts.data_ptr(),
                     keys.data_ptr(), scores.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c, k, s = counts.cpu().tolist(), keys.cpu().tolist(), scores.cpu().tolist()
    return [[(gi.key(k[i * stride + j]), s[i * stride + j]) for j in range(c[i])] for i in range(len(queries))]


def _check_dictionary(words, g, queries, n_grams):
    gi = ssl.WideStringIndex(words, 1, None, gram_size=g)
    oi = OracleIndexG(words, 1, None, g=g, wide=True)
    try:
        assert gi.lib_size() == oi.lib_size() == n_grams
        for thr, limit in [(0.0, 7), (0.3, 100), (0.6, 3)]:
            want = [oi.score(q, thr, limit) for q in queries]
            for how, got in (("score_batch", gi.score_batch(queries, thr, limit)),
                             ("search_device", _device_answers(gi, queries, thr, limit))):
                for q, a, b in zip(queries, got, want):
                    assert_exact(a, b, f"g={g} {how} q={[hex(ord(c)) for c in q]} thr={thr} limit={limit}")
        assert any(oi.score(q, 0.0, 7) for q in queries)
    finally:
        gi.dispose()


def test_gram_dictionary_chain_wraps_g1():
    """Seven code points in a 16-slot table, homes 14 and 15: the chain is slots 14, 15, 0..4."""
    present, inside, outside = hc.g1_chain()
    rng = random.Random(3)
    words = sorted({hc.text(rng.choices(present, k=rng.randint(2, 9))) for _ in range(60)})
    words += [chr(c) for c in present[:3]]  # short terms: no grams of theirs in the dictionary
    assert {c for w in words for c in w} == {chr(c) for c in present}
    queries = []
    for i in range(40):
        pool = present + (inside if i % 3 else []) + (outside if i % 3 != 1 else [])
        queries.append(hc.text(rng.choices(pool, k=rng.randint(1, 12))))
    queries += [hc.text(inside), hc.text(outside), hc.text(present), hc.text(inside[:1] + present + outside[:1])]
    queries += [w for w in words[:5]]
    _check_dictionary(words, 1, queries, len(present))


def test_gram_dictionary_chain_wraps_g2():
    """About 100 grams homing into the last 8 of 256 slots: one chain of 100 slots across the table's end."""
    terms, grams, inside, outside = hc.g2_chain()
    words = [hc.text(t) for t in terms]
    rng = random.Random(4)
    queries = list(words[:8])
    for i in range(40):
        t = list(rng.choice(terms))
        a, b = rng.choice(inside if i % 2 else outside)  # an absent gram in the middle, and around it
        p = rng.randrange(1, len(t))
        queries.append(hc.text(t[:p] + [a, b] + t[p:]))
    queries += [hc.text([a, b]) for a, b in inside + outside]
    queries += [hc.text(list(inside[0]) + list(outside[0]) + terms[0])]
    _check_dictionary(words, 2, queries, len(grams))


# ---- the count sketch -----------------------------------------------------------------------
PLANT = "0123456789.%$@"
LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
LIMIT = 100
BATCH = 17  # above the 16 queries of the latency path


def _grams(s):
    return {s[i:i + 3] for i in range(len(s) - 2)}


class Planter:
    """Queries with pairwise disjoint, unrepeated grams, and terms with an exact number of one query's
    grams and none of any other's."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.qgrams, self.terms = set(), set()

    def query(self, length):
        while True:
            q = "".join(self.rng.choices(PLANT, k=length))
            g = _grams(q)
            if len(g) == length - 2 and not g & self.qgrams and not any(g & _grams(t) for t in self.terms):
                self.qgrams |= g
                return q

    def term(self, q, hits):
        own = _grams(q)
        while True:
            s = self.rng.randrange(len(q) - hits - 1)
            body = q[s:s + hits + 2]
            pad = "".join(self.rng.choices(PLANT, k=max(0, 6 - len(body)) + self.rng.randint(1, 3)))
            t = body + pad if self.rng.random() < 0.5 else pad + body
            g = _grams(t)
            if len(g & own) == hits and not g & (self.qgrams - own) and t not in self.terms:
                self.terms.add(t)
                return t


class Group:
    def __init__(self, name, query, plan, cmins, wraps=False, crowded=False):
        self.name, self.query, self.plan, self.cmins = name, query, plan, cmins  # plan: {long-term id: (term, hits)}
        self.wraps, self.crowded = wraps, crowded

    def thr(self, cmin):
        """A threshold whose first passing count is cmin: between (cmin - 1) / n and cmin / n."""
        return 0.0 if cmin == 1 else (cmin - 0.5) / (len(self.query) - 2)


def _library(n_long, groups, seed, weighted, short=()):
    rng = random.Random(seed)
    planted = {i: t for g in groups for i, (t, _) in g.plan.items()}
    assert len(planted) == sum(len(g.plan) for g in groups) and max(planted) < n_long
    seen, words = set(planted.values()), []
    for i in range(n_long):
        w = planted.get(i)
        while w is None or (i not in planted and w in seen):
            w = "".join(rng.choices(LETTERS, k=rng.randint(8, 12)))
        seen.add(w)
        words.append(w.encode())
    words += [s.encode() for s in short]
    wts = [1.0 + 0.25 * (i % 4) for i in range(len(words))] if weighted else None
    return words, wts


def _lean_groups(seed=21):
    p = Planter(seed)
    T = hc.LEAN_CELLS

    def group(name, cells, cmins, qlen=40, **kw):
        q = p.query(qlen)
        return Group(name, q, {i: (p.term(q, h), h) for i, h in cells.items()}, cmins, **kw)

    crowd = {}
    for j in range(12):
        crowd[1000 + 8 * j] = 3
        crowd[1000 + 8 * j + T] = 3
    return [
        group("a", {40: 6, 40 + T: 5}, [2, 3, 5, 6, 7, 11, 12]),
        group("b", {104 + T: 9, 104 + 2 * T: 3}, [2, 3, 4, 9, 10, 12, 13]),
        group("c", {200: 4, 200 + T: 4}, [2, 4, 5, 8, 9]),
        group("d", {304: 8, 304 + 2 * T: 7}, [2, 7, 8, 9, 15]),
        group("e", {400 + T: 8, 400 + 2 * T: 8}, [2, 3, 8, 9, 15], wraps=True),
        group("f", {504: 16, 504 + T: 3, 505 + 2 * T: 5}, [2, 3, 5, 6, 15], wraps=True),
        group("g", {607: 16, 607 + T: 3, 608: 5}, [2, 3, 5, 6, 15], wraps=True),
        group("h", {704: 5, 704 + T: 4, 704 + 2 * T: 3}, [2, 3, 4, 5, 6, 12, 13]),
        group("ones_1_1", {800: 1, 800 + T: 1}, [1, 2, 3], qlen=20),
        group("ones_1_4", {904: 1, 904 + 2 * T: 4}, [1, 2, 4, 5], qlen=20),
        group("ones_crowd", crowd, [1, 2], qlen=20, crowded=True),
    ]


def _full_groups(seed=13):
    p = Planter(seed)
    F = hc.FULL_CELLS

    def group(name, cells, cmins, **kw):
        q = p.query(40)
        return Group(name, q, {i: (p.term(q, h), h) for i, h in cells.items()}, cmins, **kw)

    return [
        group("a", {40: 6, F + (40 ^ 1): 5}, [1, 2, 3, 5, 6, 7, 11, 12]),
        group("c", {200: 4, F + (200 ^ 1): 4}, [2, 4, 5, 8, 9]),
        group("e", {400: 8, F + (400 ^ 1): 8}, [2, 3, 8, 9, 15], wraps=True),
        group("f", {504: 16, F + (504 ^ 1): 3, 505: 5}, [2, 3, 5, 6, 15], wraps=True),
        group("g", {F + (607 ^ 1): 16, 607: 3, 608: 5}, [2, 3, 5, 6, 15], wraps=True),
    ]


LEAN_GROUPS, FULL_GROUPS = _lean_groups(), _full_groups()


LEAN_LONG, FULL_LONG = 3 * hc.LEAN_CELLS + 64, 2 * hc.FULL_CELLS


@pytest.mark.parametrize("groups,cell,n_long", [(LEAN_GROUPS, hc.lean_cell, LEAN_LONG), (FULL_GROUPS, hc.full_cell, FULL_LONG)],
                         ids=["lean", "full"])
def test_planted_groups_are_what_they_claim(groups, cell, n_long):
    """On the CPU (marked gpu with its file): one cell per group (and the next cell for the carry's
    neighbour), the hit counts, no gram shared with another group's query, and what the sketch sees
    with the strays of the chunk edges (sketch_view): only the groups meant to wrap pass 15, and tier
    1a's group d holds exactly 15."""
    view = sketch_view(_library(n_long, groups, 5, False)[0], n_long, [g.query for g in groups], cell)
    for g in groups:
        assert (view[g.query] > hc.CELL_MAX) == g.wraps, (g.name, view[g.query])
        if g.name == "d":
            assert view[g.query] == hc.CELL_MAX
        own = _grams(g.query)
        assert len(own) == len(g.query) - 2 <= 38
        cells = {}
        for i, (t, h) in g.plan.items():
            assert len(t) >= 6 and set(t) <= set(PLANT) and len(_grams(t) & own) == h
            cells.setdefault(cell(i), []).append(h)
            for other in groups:
                assert other is g or not _grams(t) & _grams(other.query), (g.name, other.name)
        shared = [hs for hs in cells.values() if len(hs) > 1]
        assert shared, g.name
        if g.crowded:
            assert sum(map(sum, shared)) > 64 and all(sum(hs) <= hc.CELL_MAX for hs in shared)
        else:
            assert len(shared) == 1 and g.wraps == (sum(shared[0]) > hc.CELL_MAX), (g.name, shared)
        if g.name in "fg":
            (c0,) = [c for c, hs in cells.items() if len(hs) > 1]
            assert cells[c0 + 1] == [5] and max(shared[0]) == 16 and (c0 % 8 == 7) == (g.name == "g")
        # one part: the query's postings are below every part target, and its chunks (at most two per
        # list) below the smallest part cap, part_ones' quarter of the sketch cap
        postings = sum(h for _, h in g.plan.values())
        assert postings <= (hc.SKETCH_CAP * 5 // 8) >> 2
        if 1 in g.cmins and cell is hc.lean_cell:  # (the full kernel counts cmin 1 exactly)
            assert 2 * (len(g.query) - 2) <= (hc.SKETCH_CAP // 4) >> 2


def sketch_view(words, n_long, queries, cell):
    """What the sketch counts for each query when its lists are one part: {query: the largest cell
    sum}. The postings are the gram lists in gram-code order, term ids ascending in each; a list is
    staged in the 16-byte chunks (4 ids, aligned to the array) that cover it, and the add pass counts
    every id of a chunk, so up to 3 ids of the neighbouring lists at each end are counted too (never
    an undercount; the candidate pass masks them out). Those strays are planted terms themselves:
    their grams sort before every letter's."""
    lists = {}
    for i, w in enumerate(words[:n_long]):
        for g in {w[j:j + 3] for j in range(len(w) - 2)}:
            lists.setdefault(g, []).append(i)
    post, off = [], {}
    for g in sorted(lists):
        off[g] = len(post)
        post += lists[g]
    out = {}
    for q in queries:
        sums = {}
        for g in _grams(q):
            g = g.encode()
            if g in off:
                for c in range(off[g] >> 2, (off[g] + len(lists[g]) + 3) >> 2):
                    for t in post[4 * c:4 * c + 4]:
                        sums[cell(t)] = sums.get(cell(t), 0) + 1
        out[q] = max(sums.values())
    return out


class SketchLib:
    def __init__(self, n_long, groups, weighted, short=()):
        from oracle_py import OracleIndex
        self.words, self.wts = _library(n_long, groups, 5, weighted, short)
        self.gi = ssl.StringIndex(self.words, 1, self.wts)
        self.oi = OracleIndex(self.words, 1, self.wts)
        self.gi.set_timing(True)
        ns = len(short)
        assert self.gi.size() == n_long + ns
        for g in groups:  # a planted term's long-term id is its position
            for i, (t, _) in g.plan.items():
                assert self.gi.term(ns + i) == t.encode(), (g.name, i)
        self._want = {}

    def want(self, q, thr):
        if (q, thr) not in self._want:
            self._want[(q, thr)] = self.oi.score(q, thr, LIMIT)
        return self._want[(q, thr)]

    def run(self, g, cmin, copies):
        q, thr = g.query.encode(), g.thr(cmin)
        want = self.want(q, thr)
        got = self.gi.score_batch([q] * copies, thr, LIMIT)
        st = self.gi.last_stats()
        for a in got:
            assert_exact(a, want, f"group {g.name} cmin {cmin} thr {thr}")
        return st, want


@pytest.fixture(scope="module", params=["one_weight", "weighted"])
def lean_lib(request):
    lib = SketchLib(LEAN_LONG, LEAN_GROUPS, request.param == "weighted")
    lib.weighted = request.param == "weighted"
    yield lib
    lib.gi.dispose()


@pytest.mark.parametrize("g", LEAN_GROUPS, ids=lambda g: g.name)
def test_tier1a_cells_shared_by_planted_terms(lean_lib, g):
    for cmin in g.cmins:
        st, want = lean_lib.run(g, cmin, BATCH)
        where = (g.name, cmin, st)
        survivors = [(t, h) for t, h in g.plan.values() if h >= cmin]
        assert {k for k, _ in want} == {t.encode() for t, _ in survivors}, "the oracle's answer is the planted terms'"
        assert st["tier2_queries"] == 0 and st["general_queries"] == 0 and st["full_queries"] == 0, where
        handed = g.wraps or g.crowded  # (sketch_view: the strays push no other group past 15)
        if cmin >= 3:  # the main tier-1a launch
            assert st["heavy_queries"] == 0, where
            assert st["handover_queries"] == (BATCH if handed else 0), where
            assert st["fast_queries"] == BATCH, where
        else:  # the heavy list: cmin 2, and threshold 0 (part_ones, or cmin 2 beside the rank lists)
            assert st["heavy_queries"] == BATCH, where
            assert st["handover_queries"] == (BATCH if handed else 0), where


def test_tier1a_two_batches_in_flight(lean_lib):
    """search_device_async: two batches of every group's query queued before either is waited for."""
    groups = [g for g in LEAN_GROUPS if len(g.query) == 40]
    qs = [g.query.encode() for g in groups] * 3
    gi = lean_lib.gi
    raw = torch.tensor(list(b"".join(qs)), dtype=torch.uint8, device=DEV)
    offs = [0]
    for q in qs:
        offs.append(offs[-1] + len(q))
    off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    calls = []
    for cmin in (3, 6):
        thr = groups[0].thr(cmin)
        counts = torch.full((len(qs),), -1, dtype=torch.int32, device=DEV)
        keys = torch.zeros(len(qs) * LIMIT, dtype=torch.int32, device=DEV)
        scores = torch.zeros(len(qs) * LIMIT, dtype=torch.float32, device=DEV)
        t = gi.search_device_async(raw.data_ptr(), off.data_ptr(), len(qs), thr, LIMIT, LIMIT, counts.data_ptr(),
                                   keys.data_ptr(), scores.data_ptr(), stream)
        calls.append((t, thr, counts, keys, scores))
    for t, thr, counts, keys, scores in reversed(calls):
        gi.wait_device(t)
        c, k, s = counts.cpu().tolist(), keys.cpu().tolist(), scores.cpu().tolist()
        for i, q in enumerate(qs):
            got = [(gi.key(k[i * LIMIT + j]), s[i * LIMIT + j]) for j in range(c[i])]
            assert_exact(got, lean_lib.want(q, thr), f"async q={q!r} thr={thr}")


@pytest.fixture(scope="module", params=["one_weight", "weighted"])
def full_lib(request):
    # one short term: its id comes before the long terms' and leaves their long-term ids alone
    lib = SketchLib(FULL_LONG, FULL_GROUPS, request.param == "weighted", short=("Z9Z",))
    yield lib
    lib.gi.dispose()


def _chain_group():
    """Twelve terms whose relative ids home into the last 4 slots of the full kernel's exact table.
    An unsliced wave's first part starts at bucket 0 (lo = bnext * span = 0 in wave_query) and, for a
    query of a few postings, is the whole library, so part_exact's rel = id - lo + 1 is id + 1."""
    p = Planter(31)
    q = p.query(40)
    bits = hc.FULL_SLOT_BITS
    ids = [i for i in range(FULL_LONG) if hc.exact_home(i + 1, bits) >= (1 << bits) - 4][:12]
    return Group("exact_chain", q, {i: (p.term(q, 1 + k % 3), 1 + k % 3) for k, i in enumerate(ids)}, [1])


CHAIN_GROUP = _chain_group()


@pytest.mark.parametrize("weighted", [False, True], ids=["one_weight", "weighted"])
def test_exact_table_chain_wraps(weighted):
    """wave_insert_slot at cmin 1 (threshold 0 on the latency path: the full kernel counts exactly):
    twelve relative ids with homes in the table's last 4 slots, so whatever order the lanes insert in,
    at least 8 of them probe past the end to slot 0 and on."""
    g, bits = CHAIN_GROUP, hc.FULL_SLOT_BITS
    assert len(g.plan) == 12 and all(hc.exact_home(i + 1, bits) >= (1 << bits) - 4 for i in g.plan)
    lib = SketchLib(FULL_LONG, [g], weighted, short=("Z9Z",))
    try:
        st, want = lib.run(g, 1, 3)
        assert {k for k, _ in want} == {t.encode() for t, _ in g.plan.values()}
        assert st["fast_queries"] == 3 and st["general_queries"] == 0 and st["tier2_queries"] == 0, st
    finally:
        lib.gi.dispose()


@pytest.mark.parametrize("g", FULL_GROUPS, ids=lambda g: g.name)
def test_full_kernel_cells_shared_by_planted_terms(full_lib, g):
    """Batches of 3 take the latency path: the full kernel alone, one unsliced wave per query."""
    for cmin in g.cmins:
        st, want = full_lib.run(g, cmin, 3)
        where = (g.name, cmin, st)
        assert {k for k, _ in want} == {t.encode() for t, h in g.plan.values() if h >= cmin}
        assert st["fast_queries"] == 3 and st["general_queries"] == 0 and st["tier2_queries"] == 0, where
        assert st["heavy_queries"] == 0 and st["full_queries"] == 0 and st["handover_queries"] == 0, where
