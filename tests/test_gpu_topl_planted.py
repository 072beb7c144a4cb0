"""Tier 1's running top-L (wave_flush, wave_sort64, wave_trim, wave_select, term_pairs' w_max prune,
raised_cmin's tie rule, emit_rank_prefix's key set, k_merge's join) on the planted libraries of
tests/topl_cases.py, exact against the oracle (keys, order, fp32 bits, counts) through scoreBatch and
ngsSearchDevice, with ngsLastError(1) == 0 after every call and the route asserted from ngsLastStats:

  main     spread families, threshold 0.3 (cmin 3), 17 queries or more: the main launch and k_emit<false>;
           fast_queries == n, no heavy, full, handed-over, tier-2 or general query, survivors == the sum of
           the families' surviving terms;
  heavy    the same queries at threshold 0.2 (cmin 2): the heavy list and k_emit<true> (wave_select);
           heavy_queries == n, none handed over;
  handover dense families, threshold 0.3, 17 queries or more: every part of 64 candidates' worth hands the
           query to sliced tier 1b and k_merge; handover_queries == n;
  latency  up to 16 queries: tier 1b alone (wave_emit, raised_cmin, wave_flush<false>), one wave per query on
           library u (8 skip buckets) and slices with k_merge on the others (asserted from the digest);
           heavy_queries == 0 even at cmin 2. scoreBatch alone takes it: ngsSearchDevice runs every batch
           through the batch path. A list of more than 135 postings gives an index 16 buckets or more, so
           library u reaches refills, the descending prune and the winning tie at tau through families whose
           records come from several keys per word (M, Uo, Ut);
  rank     library r at threshold 0: digest bit 8, the heavy list, and the answers of the same rows built
           under NGS_NO_RANK_LISTS=1.

Queries of different families share every batch (every library holds two families or more). tests/test_topl_cases.py proves on the CPU what the
families are and which branches they reach. The index must report the skip-table geometry and the flag
word (ngsIndexDigest words 2, 7 and 16) that the CPU facts were proved at.
"""
import ctypes as C
import os

import pytest

import stringsearchlib_amd as ssl
import topl_cases as tc
from oracle_py import OracleIndex
from stringsearchlib_amd import _native
from test_gpu_fast_planted import SMALL, Leg
from test_gpu_parity import assert_exact

pytestmark = pytest.mark.gpu

ROUTE_KEYS = ("fast_queries", "heavy_queries", "full_queries", "handover_queries", "tier2_queries", "general_queries",
              "survivors")


def _digest(gi):
    out = (C.c_uint64 * 17)()
    assert _native.lib().ngsIndexDigest(gi.handle, out, 17) == 17
    return (out[2], out[7]), out[16]


class TopLeg(Leg):
    """One planted library on the device with its oracle (Leg's device_answers and answer cache)."""

    def __init__(self, lib, oracle=True):
        self.lib, self.wide = lib, False
        words = lib.encoded()
        self.gi = ssl.StringIndex(words, lib.row_size, lib.weights)
        self.oi = OracleIndex(words, lib.row_size, lib.weights) if oracle else None
        self.enc = lambda q: q.encode()
        self.gi.set_timing(True)
        self.geometry, self.flags = _digest(self.gi)
        self._want, self._keys = {}, {}
        self.surv = {f.query: tc.survivors(f) for f in lib.families}

    def answers(self, queries, thr, limit):
        """[(entry point, answers, statistics)] with the kernels' error bits checked."""
        out = []
        for how in ("score_batch", "search_device"):
            _native.lib().ngsLastError(1)
            if how == "score_batch":
                got = self.gi.score_batch([q.encode() for q in queries], thr, limit)
            else:
                got = self.device_answers(queries, thr, limit)
            err = _native.lib().ngsLastError(1)
            assert err == 0, (how, self.lib.name, thr, limit, err)
            out.append((how, got, self.gi.last_stats()))
        return out

    def check(self, queries, thr, limit, route=None):
        assert len(queries) <= SMALL or len(queries) >= 17
        n = len(queries)
        for how, got, st in self.answers(queries, thr, limit):
            where = f"{self.lib.name} {how} n={n} thr={thr} limit={limit}"
            for q, a in zip(queries, got):
                assert_exact(a, self.want(q, thr, limit), f"{where} q={q!r}")
            seen = {k: st[k] for k in ROUTE_KEYS}
            print(where, route, seen)
            assert st["tier2_queries"] == 0 and st["general_queries"] == 0 and st["full_queries"] == 0, (where, seen)
            if route == "main":
                assert st["fast_queries"] == n and st["heavy_queries"] == 0 and st["handover_queries"] == 0, (where, seen)
                assert st["survivors"] == sum(self.surv[q] for q in queries), (where, seen)
            elif route == "heavy":
                assert st["heavy_queries"] == n and st["handover_queries"] == 0, (where, seen)
            elif route == "handover":
                assert st["handover_queries"] == n, (where, seen)
            elif route == "latency":  # no heavy list is made there, even at cmin 2
                if how == "score_batch":
                    assert st["heavy_queries"] == 0 and st["handover_queries"] == 0, (where, seen)
            else:
                assert route is None


MAKERS, SPREAD = tc.MAKERS, tc.SPREAD


@pytest.fixture(scope="module")
def legs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = TopLeg(MAKERS[name]())
        return made[name]

    yield get
    for leg in made.values():
        leg.gi.dispose()


def big_batch(lib):
    """Every family's query, repeated until there are 17."""
    qs = [f.query for f in lib.families]
    return qs * -(-17 // len(qs))


def small_batches(lib):
    """Every family's query in batches of at most 16, each beside other families' (the last one filled up
    from the front)."""
    qs = [f.query for f in lib.families]
    out = [qs[i:i + SMALL] for i in range(0, len(qs), SMALL)]
    if len(out) > 1 and len(out[-1]) < 4:
        out[-1] = out[-1] + qs[:4]
    return out


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_geometry_flags_and_term_ids(legs, name):
    leg = legs(name)
    m = leg.lib.model()
    assert leg.geometry == tc.skip_buckets(m.n_long, max(map(len, m.lists))), name
    assert leg.flags == tc.flag_word(m), name
    assert leg.gi.num_keys() == len(m.keys)
    for i in (0, 1, len(m.terms) // 2, len(m.terms) - 1):  # a long-term id is the model's
        assert leg.gi.term(i) == bytes(m.terms[i]), (name, i)
    # the latency path: slices and k_merge from 16 skip buckets on, one wave per query below
    assert (leg.geometry[0] // 8 <= 1) == (name == "u")


@pytest.mark.parametrize("name", SPREAD)
def test_main_launch(legs, name):
    leg = legs(name)
    qs = big_batch(leg.lib)
    for limit in tc.limits_of(name):
        leg.check(qs, 0.3, limit, "main")


@pytest.mark.parametrize("name", SPREAD)
def test_heavy_list(legs, name):
    leg = legs(name)
    qs = big_batch(leg.lib)
    for limit in tc.limits_of(name):
        leg.check(qs, 0.2, limit, "heavy")


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_latency_path(legs, name):
    leg = legs(name)
    for limit in tc.limits_of(name):
        for thr in (0.3, 0.2):
            for qs in small_batches(leg.lib):
                leg.check(qs, thr, limit, "latency")


def test_dense_families_hand_over_to_sliced_tier_1b(legs):
    leg = legs("d")
    wide = [f.query for f in leg.lib.families if f.n >= 192]
    rest = [f.query for f in leg.lib.families if f.n < 192]
    wide = wide * -(-17 // len(wide))
    assert len(wide) >= 17 and rest
    for limit in tc.LIMITS:
        leg.check(wide, 0.3, limit, "handover")
        leg.check(wide + rest, 0.3, limit)   # (B3's 128 targets may fit two parts of 64)
        leg.check(wide + rest, 0.2, limit)   # the heavy list's hand-overs and their k_merge


_BASE = {}


def base_answers(leg):
    """A twin's base library's device answers per (threshold, limit, batch): what the twin must give, bit for bit."""
    name = leg.lib.name
    if name not in _BASE:
        out = {}
        for thr in (0.3, 0.2):
            for limit in (1, 64, 128):
                for tag, qs in (("big", big_batch(leg.lib)), ("small", small_batches(leg.lib)[0])):
                    out[(thr, limit, tag)] = [(how, got) for how, got, _ in leg.answers(qs, thr, limit)]
                    for q, a in zip(qs, out[(thr, limit, tag)][0][1]):
                        assert_exact(a, leg.want(q, thr, limit), f"{name} thr={thr} limit={limit} {tag} q={q!r}")
        _BASE[name] = out
    return _BASE[name]


@pytest.mark.parametrize("name,kind", tc.TWIN_CASES)
def test_flag_twins(legs, name, kind):
    """A library and far rows that flip one index-shape flag (or w_max): the same answers, key strings and fp32
    bits, on the same routes. Libraries e2, o1, n1 and a hold families of more than 256 records, so the
    flipped flag meets refills, a finite tau in term_pairs and the dedup pass on a full buffer; e2 holds T."""
    base = legs(name)
    lib = tc.twin(base.lib, kind)
    leg = TopLeg(lib, oracle=False)
    try:
        assert leg.flags == tc.flag_word(lib.model()), (name, kind, leg.flags)
        assert (leg.flags != base.flags) == (kind != "huge"), (name, kind, leg.flags)  # "huge" changes w_max alone
        for (thr, limit, tag), want in base_answers(base).items():
            qs = big_batch(base.lib) if tag == "big" else small_batches(base.lib)[0]
            for (how, got, st), (_, ref) in zip(leg.answers(qs, thr, limit), want):
                assert got == ref, (name, kind, how, thr, limit, tag)
                if tag == "big":
                    assert st["heavy_queries" if thr == 0.2 else "fast_queries"] == len(qs), (name, kind, how, thr, limit)
                    assert st["handover_queries"] == 0, (name, kind, how, thr, limit)
    finally:
        leg.gi.dispose()


@pytest.mark.parametrize("name", ["e1", "e2"])
def test_negative_weights(legs, name):
    """w_max <= 0: every score is +0, every prune bound ties, and the key rank alone cuts."""
    lib = tc.negative(legs(name).lib)
    leg = TopLeg(lib)
    try:
        assert leg.flags == tc.flag_word(lib.model())
        for limit in (1, 64, 128):
            leg.check(big_batch(lib), 0.3, limit, "main")
            leg.check(big_batch(lib), 0.2, limit, "heavy")
            leg.check(small_batches(lib)[0], 0.3, limit, "latency")
    finally:
        leg.gi.dispose()


@pytest.mark.parametrize("weight", [None, -2.0])
def test_rank_lists(weight):
    lib = tc.lib_r(weight)
    leg = TopLeg(lib)
    os.environ["NGS_NO_RANK_LISTS"] = "1"
    try:
        plain = TopLeg(lib, oracle=False)
    finally:
        del os.environ["NGS_NO_RANK_LISTS"]
    twin = TopLeg(tc.twin(lib, "weight"), oracle=False)
    try:
        assert leg.flags == 15 and plain.flags == 7 and twin.flags == 7
        qs = list(lib.queries.values()) * 6
        for limit in tc.LIMITS:
            for batch in (qs, qs[:3]):
                ours = leg.answers(batch, 0.0, limit)
                for (how, got, st), (_, ref, _), (_, tw, _) in zip(ours, plain.answers(batch, 0.0, limit),
                                                                  twin.answers(batch, 0.0, limit)):
                    where = f"r weight={weight} {how} n={len(batch)} limit={limit}"
                    for q, a in zip(batch, got):
                        assert_exact(a, leg.want(q, 0.0, limit), f"{where} q={q!r}")
                    assert got == ref and got == tw, where
                    if len(batch) >= 17:
                        assert st["heavy_queries"] == len(batch) and st["handover_queries"] == 0, (where, st)
    finally:
        for x in (leg, plain, twin):
            x.gi.dispose()
