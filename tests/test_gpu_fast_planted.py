"""Tier 2 (k_fast / fast_one: one 512-thread block per query) on planted libraries, exact against the
oracle (keys, order, fp32 bits, counts) through scoreBatch and ngsSearchDevice, once as a batch of at
most 16 queries (the latency path) and once as 17 or more. tests/fast_cases.py plants the libraries and
states what fast_one makes of every query; tests/test_fast_cases.py proves that on the CPU.

  P  the planner's three outcomes: one part (p_total <= 4,096), the greedy cut into whole-bucket
     parts (with runs of empty buckets before, between and behind), and buckets over the cap that go
     to term-id sub-parts, alternating with whole-bucket parts up to six times in one query; at limits
     200 and 1,024, which route every query to tier 2. Then the u8 count at 255: 257-character queries
     (one gram 255 times, two grams 128 + 127 times, 255 grams once each: ng = 255 fills every entry of
     the per-gram arrays) at limits 100 and 1,024, their one-character variants (252..254 beside 255)
     and 258-character controls, which k_fast passes on to the general path. And a chain of table
     entries whose relative ids home into the last four slots with a part base that is not 0;
  T  table_insert's chain across the table's end: 19 relative ids homing into slots 8188..8191, 3
     leading into them and 11 homing into the slots 0..10 that the wrapped chain takes, each term with
     a hit count of its own, at thresholds that cut through the counts;
  D  the candidate buffer: at least 6,144 scored terms per query, so two or three flushes, over keys
     with two aliases whose records fall into different flushes: the better one first, second, both
     alike, and a +0 beside a positive score;
  W  the planner's outcomes once more on a wide index of gram size 2 (dictionary lookup, 4-byte
     characters); "over" cannot occur there (test_fast_cases.test_w_classes says why).

After every call: ngsLastError is 0 (the kernel's error bits: 1 a full table, 2 a flush loop, 4 the
sub-part guard), and ngsLastStats says that every query was listed for tier 2 and finished there, with
lists = the sum of ng and postings = the sum of p_total over the batch, which fast_one adds once per
query whatever its parts. The 258-character controls are listed for tier 2 by tier 1 as well
(tier2_queries counts the list, test_gpu_tiers.test_tier2_gram_count_edges) and show in
general_queries, not in fast_queries.

The index must report the skip-table geometry the CPU facts were proved at (fast_cases.P_GEOM, W_GEOM,
D_GEOM): a change of geometry fails here instead of turning "over" queries into "multi" ones.
"""
import ctypes as C
import struct

import pytest
import torch

import fast_cases as fc
import stringsearchlib_amd as ssl
from oracle_py import OracleIndex, OracleIndexG
from stringsearchlib_amd import _native
from test_gpu_parity import assert_exact

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SMALL = 16  # kSmallBatch: up to this many queries take the latency path


def _geometry(gi):
    out = (C.c_uint64 * 17)()
    assert _native.lib().ngsIndexDigest(gi.handle, out, 17) == 17
    return out[2], out[7]


class Leg:
    """One library on the device with its oracle; oracle answers computed once per (query, thr, limit)."""

    def __init__(self, rows, row_size=1, weights=None, wide=False):
        self.wide = wide
        if wide:
            self.gi = ssl.WideStringIndex(rows, row_size, weights, gram_size=2)
            self.oi = OracleIndexG(rows, row_size, weights, g=2, wide=True)
            self.enc = lambda q: q
        else:
            words = [r.encode() for r in rows]
            self.gi = ssl.StringIndex(words, row_size, weights)
            self.oi = OracleIndex(words, row_size, weights)
            self.enc = lambda q: q.encode()
        self.gi.set_timing(True)
        self.geometry = _geometry(self.gi)
        assert self.gi.size() == len(rows)
        for i in (0, 1, len(rows) // 2, len(rows) - 2, len(rows) - 1):  # a long-term id is a position
            assert self.gi.term(i) == self.enc(rows[i]), i
        self._want, self._keys = {}, {}

    def want(self, q, thr, limit):
        if (q, thr, limit) not in self._want:
            self._want[(q, thr, limit)] = self.oi.score(self.enc(q), thr, limit)
        return self._want[(q, thr, limit)]

    def key(self, k):
        if k not in self._keys:
            self._keys[k] = self.gi.key(k)
        return self._keys[k]

    def device_answers(self, queries, thr, limit):
        if self.wide:
            units = [struct.pack(f"<{len(q)}I", *map(ord, q)) for q in queries]
        else:
            units = [q.encode() for q in queries]
        offs = [0]
        for u in units:
            offs.append(offs[-1] + len(u))
        raw = torch.frombuffer(bytearray(b"".join(units)), dtype=torch.uint8).to(DEV)
        off = torch.tensor(offs, dtype=torch.int64, device=DEV)
        stride = max(1, min(limit, self.gi.num_keys()))
        counts = torch.zeros(len(queries), dtype=torch.int32, device=DEV)
        keys = torch.zeros(len(queries) * stride, dtype=torch.int32, device=DEV)
        scores = torch.zeros(len(queries) * stride, dtype=torch.float32, device=DEV)
        _native.lib().ngsLastError(1)
        self.gi.search_device(raw.data_ptr(), off.data_ptr(), len(queries), thr, limit, stride, counts.data_ptr(),
                              keys.data_ptr(), scores.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        c, k, s = counts.cpu().tolist(), keys.cpu().tolist(), scores.cpu().tolist()
        return [[(self.key(k[i * stride + j]), s[i * stride + j]) for j in range(c[i])] for i in range(len(queries))]

    def check(self, queries, thr, limit, plans, general=False):
        """Both entry points: exact answers, no kernel error, the route and fast_one's own counts."""
        assert len(queries) <= SMALL or len(queries) >= 17
        for how in ("score_batch", "search_device"):
            if how == "score_batch":
                got = self.gi.score_batch([self.enc(q) for q in queries], thr, limit)
            else:
                got = self.device_answers(queries, thr, limit)
            err = _native.lib().ngsLastError(1)
            st = self.gi.last_stats()
            where = f"{how} n={len(queries)} thr={thr} limit={limit}"
            for q, a in zip(queries, got):
                assert_exact(a, self.want(q, thr, limit), f"{where} q={q[:40]!r} len={len(q)}")
            assert err == 0, (where, err)
            n = len(queries)
            route = {k: st[k] for k in ("tier2_queries", "fast_queries", "general_queries", "lists", "postings")}
            print(where, route)
            assert st["tier2_queries"] == n, (where, route)
            if general:
                assert st["general_queries"] == n and st["fast_queries"] == 0, (where, route)
                continue
            assert st["fast_queries"] == n and st["general_queries"] == 0, (where, route)
            assert st["lists"] == sum(plans[q].ng for q in queries), (where, route)
            assert st["postings"] == sum(plans[q].p_total for q in queries), (where, route)


# ---- P ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def P():
    lib = fc.LibP()
    leg = Leg(lib.rows)
    yield lib, leg
    leg.gi.dispose()


def test_p_geometry(P):
    lib, leg = P
    assert leg.geometry == fc.P_GEOM
    fc.check_geometry(lib.n_long, *leg.geometry)
    for i, (t, _) in lib.chain_plan.items():
        assert leg.gi.term(i) == t.encode()
    for i in range(fc.P_BASE, fc.P_ROWS):
        assert leg.gi.term(i) == lib.rows[i].encode()


@pytest.mark.parametrize("limit", [200, 1024])
@pytest.mark.parametrize("thr", fc.P_THRESHOLDS)
def test_p_planner_outcomes(P, thr, limit):
    """One part, whole-bucket parts, oversized buckets and their alternation; the band's empty runs; the
    second chain (rel = id - lo + 1 with lo != 0) rides on the first "multi" query."""
    lib, leg = P
    qs = lib.all_queries()
    assert len(qs) >= 17
    small = qs[::2] + [lib.chain_query]
    assert {lib.plans[q].cls for q in small} == {"one", "multi", "over"}
    leg.check(small, thr, limit, lib.plans)
    leg.check(qs, thr, limit, lib.plans)


def test_p_second_chain_is_scored(P):
    """The oracle's answer to the chain query at threshold 0 holds every planted term of the second chain
    (a limit of 1,024 is above what the query scores at 3 hits or more of its grams)."""
    lib, leg = P
    n = len(lib.chain_query) - 2
    thr = 2.5 / n
    keys = {k for k, _ in leg.want(lib.chain_query, thr, 1024)}
    assert len(keys) < 1024 and {t.encode() for t, _ in lib.chain_plan.values()} <= keys
    leg.check([lib.chain_query] * 3, thr, 1024, lib.plans)


@pytest.mark.parametrize("limit", [100, 1024])
@pytest.mark.parametrize("thr", fc.P_THRESHOLDS)
def test_p_count_255(P, thr, limit):
    """257 characters: the u8 count reaches 255 in one add of 255, in 128 + 127, and in 255 single adds
    (ng = 255); the variants leave 252..254 beside it."""
    lib, leg = P
    qs = lib.long_queries
    if thr == 1.0:
        for q in qs[:3]:  # the row itself scores 255 / 255
            assert q.encode() in [k for k, _ in leg.want(q, thr, limit)]
    leg.check(qs, thr, limit, lib.plans)
    leg.check(qs * 3, thr, limit, lib.plans)


def test_p_controls_go_general(P):
    """258 characters (256 grams): k_fast hands them to the general path."""
    lib, leg = P
    leg.check(lib.controls, 0.3, 100, None, general=True)
    leg.check(lib.controls * 6, 0.3, 1024, None, general=True)


def test_small_batch_after_a_larger_small_batch(P):
    """The latency path's statistics: its block has a slot per query (q mod 256) and ngsLastStats sums all
    of them, so k_prep has to zero the slots the context's last small batch added to beside the new
    batch's own. Before it did, a batch of 3 after one of 14 reported 14 fast queries and the other 11's
    lists and postings."""
    lib, leg = P
    qs = lib.queries["one"]
    leg.check(qs[:8], 0.3, 200, lib.plans)
    leg.check(qs[5:7], 0.3, 200, lib.plans)
    leg.check(qs[:1], 0.3, 200, lib.plans)
    leg.check(qs[2:6], 0.3, 200, lib.plans)


# ---- T ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def T():
    lib = fc.LibT()
    leg = Leg(lib.rows)
    for i, (t, _) in lib.plan.items():
        assert leg.gi.term(i) == t.encode(), i
    yield lib, leg
    leg.gi.dispose()


@pytest.mark.parametrize("thr", fc.T_THRESHOLDS)
def test_t_chain_wraps(T, thr):
    lib, leg = T
    pl = fc.plan(lib.lists, lib.query, *leg.geometry)
    assert pl.cls == "one"
    want = leg.want(lib.query, thr, fc.T_LIMIT)
    assert {k for k, _ in want} == {t.encode() for t, h in lib.plan.values() if h / 38 >= thr}
    plans = {lib.query: pl}
    leg.check([lib.query] * 3, thr, fc.T_LIMIT, plans)
    leg.check([lib.query] * 17, thr, fc.T_LIMIT, plans)


# ---- D ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def D():
    lib = fc.LibD()
    leg = Leg(lib.words, 3, lib.weights)
    lib.plans = {q: fc.plan(lib.lists, q, *fc.D_GEOM) for q in lib.queries}
    yield lib, leg
    leg.gi.dispose()


def test_d_geometry_and_term_ids(D):
    lib, leg = D
    assert leg.geometry == fc.D_GEOM
    for i in range(0, len(lib.words), 997):
        assert leg.gi.term(i) == lib.words[i].encode()
    assert leg.gi.num_keys() == fc.D_KEYS


@pytest.mark.parametrize("limit", fc.D_LIMITS)
@pytest.mark.parametrize("thr", fc.D_THRESHOLDS)
def test_d_buffer_and_dedup(D, thr, limit):
    lib, leg = D
    assert len(lib.queries) >= 17
    leg.check(lib.queries[:SMALL], thr, limit, lib.plans)
    leg.check(lib.queries, thr, limit, lib.plans)


# ---- W ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def W(P):
    lib, _ = P
    rows = fc.w_rows(lib)
    leg = Leg(rows, wide=True)
    lists = fc.lists_of(rows, 2)
    plans = {q: fc.plan(lists, q, *fc.W_GEOM, 2) for q in fc.w_queries(lib)}
    yield lib, leg, plans
    leg.gi.dispose()


@pytest.mark.parametrize("limit", [200, 1024])
@pytest.mark.parametrize("thr", fc.P_THRESHOLDS)
def test_w_planner_outcomes(W, thr, limit):
    lib, leg, plans = W
    assert leg.geometry == fc.W_GEOM
    fc.check_geometry(fc.W_ROWS, *leg.geometry)
    qs = fc.w_queries(lib)
    assert len(qs) >= 17 and {p.cls for p in plans.values()} == {"one", "two", "multi"}
    small = qs[:SMALL]
    assert {plans[q].cls for q in small} == {"one", "two", "multi"}
    leg.check(small, thr, limit, plans)
    leg.check(qs, thr, limit, plans)
