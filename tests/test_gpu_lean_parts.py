"""The main tier-1a launch's planner (lean_query_g: lane quotas that take all 64 lanes, parts as wide
as fit) on libraries where every width occurs, exact against the oracle through scoreBatch and
ngsSearchDevice at threshold 0.3 and limit 100.

40,000 distinct rows of 10..15 letters, each its own key and long term, so a long-term id is a row
number and the skip table has K = 16 buckets of 2,500 ids. Rows 15,000..24,999 are over the letters
N..Z, the others over A..M: 2,197 grams per alphabet, lists of about 12 postings per bucket. A query of
7..12 grams gives its lists groups of 5..9 lanes (caps of 15..27 chunks), so its parts are 1..8
buckets wide depending on how the lists' segments fall; the widths differ from part to part.
  plain      9..14-character queries cut from rows and mutated (7..12 grams, cmin 3 or 4)
  repeat     queries that repeat grams (a row's first six letters twice): a repeated gram owns a
             group of lanes per occurrence
  long       45..50-character queries of 43..48 grams, rows laid end to end: groups of 1 or 2 lanes, so
             the width is pinned to one bucket and a bucket of more than 3 or 6 chunks goes to
             sub-parts
  band       queries over N..Z: every list is empty over the six leading and the six trailing
             buckets (and A..M queries over the four in the middle)
  hot        a second library in which the A..M rows of the odd buckets hold the gram ABC with
             probability 0.7, and independently DEF, and the rows of the even buckets with 0.05 (each
             gram in about 30 % of all rows). In a 12-character query with one of them that list gets
             about 50 lanes, a cap of about 150 chunks, which an odd bucket's ~1,750 postings overflow
             and an even bucket's ~125 do not, so the planner enters the sub-part path and returns to
             whole buckets six times per query (asserted below from the lists); queries with both,
             with a hot gram twice, and a long one with a hot gram are there too
No cmin-2 case: the main launch never sees one. Queries with cmin <= 2 (kHeavyCmin) go to the heavy
list from the start (lean_route), whose launch keeps the packed staging (lean_query); the halved cap
of cmin 2 in lean_query_g is exercised on the host only (tests/test_lean_plan_model.py).

ngsLastStats: the batch's postings and lists are the sums over its queries' non-empty lists, with
multiplicity, computed here from the rows (the counts are the route's, taken once per query whatever
its parts: a part that dropped or repeated postings shows in the answers). Every query starts on the
main launch; the main launch's own share (main_postings, main_lists) leaves out the queries it handed
over to exact counting, which the fixed-width planner handed over as well.
"""
import random

import pytest
import torch

import stringsearchlib_amd as ssl
from oracle_py import OracleIndex
from test_gpu_parity import assert_exact

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROWS, K, SPAN = 40000, 16, 2500
AM, NZ = "ABCDEFGHIJKLM", "NOPQRSTUVWXYZ"
THR, LIMIT = 0.3, 100


def _rows(hot):
    rng = random.Random(77 if hot else 76)
    seen, rows = set(), []
    for i in range(ROWS):
        letters = NZ if 15000 <= i < 25000 else AM
        while True:
            w = "".join(rng.choices(letters, k=rng.randint(10, 15)))
            for g, lo in (("ABC", 0), ("DEF", 5)) if hot and letters is AM else ():
                if rng.random() < (0.7 if (i // SPAN) & 1 else 0.05):
                    p = rng.randrange(lo, lo + 3) if lo == 0 else rng.randrange(lo, len(w) - 2)
                    w = w[:p] + g + w[p + 3:]
            if w not in seen:
                break
        seen.add(w)
        rows.append(w)
    return rows


def _grams(s):
    return [s[i:i + 3] for i in range(len(s) - 2)]


def _queries(rows, hot):
    rng = random.Random(5)
    am = [r for i, r in enumerate(rows) if not 15000 <= i < 25000]
    nz = rows[15000:25000]

    def mutate(w, letters):
        w = list(w)
        for _ in range(rng.randint(0, 2)):
            w[rng.randrange(len(w))] = rng.choice(letters)
        return "".join(w)

    def cut(pool, letters, n):
        w = rng.choice(pool)
        while len(w) < n:
            w += rng.choice(pool)
        s = rng.randrange(len(w) - n + 1)
        return mutate(w[s:s + n], letters)

    qs = [cut(am, AM, 12) for _ in range(24)]
    qs += [cut(am, AM, n) for n in (9, 10, 11, 13, 14) for _ in range(4)]
    for _ in range(8):
        w = rng.choice(am)
        qs += [w[:6] + w[:6], w[:5] + w[:5] + w[:4]]
    for _ in range(6):
        w = rng.choice(am)  # one whole row inside, so that some term reaches cmin
        qs.append((rng.choice(am) + w + rng.choice(am) + rng.choice(am) + rng.choice(am))[:rng.randint(45, 50)])
    qs += [cut(nz, NZ, n) for n in (12, 12, 12, 10, 14, 9)]
    qs += [(rng.choice(nz) * 5)[:46]]
    if hot:
        for k in range(12):  # one hot gram, the other, or both
            w = cut(am, AM, 12)
            if k % 3 != 1:
                w = "ABC" + w[3:] if k & 4 else w[:4] + "ABC" + w[7:]
            if k % 3:
                w = w[:8] + "DEF" + w[11:]
            qs.append(w)
        qs += ["ABCDEFABCDEF", (rng.choice(am) + "ABC" + rng.choice(am) + rng.choice(am) + rng.choice(am))[:47]]
    return qs


class Lib:
    def __init__(self, hot):
        self.rows = _rows(hot)
        self.words = [r.encode() for r in self.rows]
        self.queries = _queries(self.rows, hot)
        self.gi = ssl.StringIndex(self.words, 1, None)
        self.oi = OracleIndex(self.words, 1, None)
        self.gi.set_timing(True)
        assert self.gi.size() == ROWS and all(self.gi.term(i) == self.words[i] for i in (0, 1, 17000, ROWS - 1))
        self.lists = {}
        for i, r in enumerate(self.rows):
            for g in set(_grams(r)):
                self.lists.setdefault(g, []).append(i)
        self.want = [self.oi.score(q.encode(), THR, LIMIT) for q in self.queries]  # computed once, shared


@pytest.fixture(scope="module", params=["plain", "hot"])
def lib(request):
    lb = Lib(request.param == "hot")
    lb.hot = request.param == "hot"
    yield lb
    lb.gi.dispose()


def test_queries_are_what_they_claim(lib):
    """On the CPU (marked gpu with its file): every query is on the main launch's route (9 or more
    characters, cmin >= 3), the shapes named above are there, and in the hot library the two hot lists
    overflow their lanes' cap in the odd buckets and stay under it in the even ones."""
    for q in lib.queries:
        n = len(q) - 2
        assert len(q) >= 9 and min(c for c in range(1, n + 1) if c / n >= THR) >= 3, q
    assert sum(len(q) == 12 for q in lib.queries) >= 24
    assert any(len(set(_grams(q))) < len(q) - 2 for q in lib.queries)
    assert sum(len(q) >= 45 for q in lib.queries) >= 7
    assert any(w for w in lib.want) and sum(1 for w in lib.want if w) > len(lib.want) // 2
    band = [q for q in lib.queries if set(q) <= set(NZ)]
    assert len(band) >= 7
    for q in band:
        ids = [i for g in _grams(q) for i in lib.lists.get(g, [])]
        assert ids and min(ids) >= 6 * SPAN and max(ids) < 10 * SPAN
    if lib.hot:
        for g in ("ABC", "DEF"):
            q = next(q for q in lib.queries if len(q) == 12 and _grams(q).count(g) == 1 and
                     not any(h in q for h in ("ABC", "DEF") if h != g))
            lens = [len(lib.lists.get(h, [])) for h in _grams(q)]
            total = sum(lens)
            ng = sum(1 for ln in lens if ln)
            ids = lib.lists[g]
            assert 0.25 * ROWS < len(ids) < 0.35 * ROWS
            lanes = 1 + (64 - ng) * len(ids) // total  # the list's quota, or one less
            per_bucket = [sum(1 for i in ids if i // SPAN == b) for b in range(K)]
            for b in (0, 2, 4, 10, 12, 14):
                assert per_bucket[b] + 3 <= 12 * lanes, (b, per_bucket[b], lanes)  # fits 3 rounds of its lanes
            for b in (1, 3, 5, 11, 13, 15):
                assert per_bucket[b] > 12 * (lanes + 1), (b, per_bucket[b], lanes)  # over the cap


def _device_answers(gi, queries):
    raw = torch.tensor(list(b"".join(queries)), dtype=torch.uint8, device=DEV)
    offs = [0]
    for q in queries:
        offs.append(offs[-1] + len(q))
    off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    counts = torch.zeros(len(queries), dtype=torch.int32, device=DEV)
    keys = torch.zeros(len(queries) * LIMIT, dtype=torch.int32, device=DEV)
    scores = torch.zeros(len(queries) * LIMIT, dtype=torch.float32, device=DEV)
    gi.search_device(raw.data_ptr(), off.data_ptr(), len(queries), THR, LIMIT, LIMIT, counts.data_ptr(),
                     keys.data_ptr(), scores.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c, k, s = counts.cpu().tolist(), keys.cpu().tolist(), scores.cpu().tolist()
    return [[(gi.key(k[i * LIMIT + j]), s[i * LIMIT + j]) for j in range(c[i])] for i in range(len(queries))]


def _check_stats(lib, st):
    lens = [len(lib.lists.get(g, [])) for q in lib.queries for g in _grams(q)]
    where = {k: st[k] for k in ("postings", "lists", "main_postings", "main_lists", "fast_queries", "heavy_queries",
                                "full_queries", "handover_queries", "tier2_queries", "general_queries")}
    assert st["postings"] == sum(lens) and st["lists"] == sum(1 for ln in lens if ln), where
    # every query starts in the main launch; the ones it hands over (a counter that wraps, or more
    # than 64 candidates in a part: repeated grams, both hot grams in one query) are counted by tier 1b
    assert st["fast_queries"] == len(lib.queries) and st["heavy_queries"] == 0 and st["full_queries"] == 0, where
    assert st["tier2_queries"] == 0 and st["general_queries"] == 0, where
    assert 0 < st["main_lists"] <= st["lists"] and 0 < st["main_postings"] <= st["postings"], where
    assert st["handover_queries"] < len(lib.queries), where


def test_score_batch_exact(lib):
    qs = [q.encode() for q in lib.queries]
    assert len(qs) > 16  # past the latency path
    got = lib.gi.score_batch(qs, THR, LIMIT)
    st = lib.gi.last_stats()
    for q, a, b in zip(qs, got, lib.want):
        assert_exact(a, b, f"score_batch q={q!r}")
    _check_stats(lib, st)


def test_search_device_exact(lib):
    qs = [q.encode() for q in lib.queries]
    got = _device_answers(lib.gi, qs)
    st = lib.gi.last_stats()
    for q, a, b in zip(qs, got, lib.want):
        assert_exact(a, b, f"search_device q={q!r}")
    _check_stats(lib, st)
