"""The general path (k_gen_*) past one group of queries, exact against the oracle.

finish_search cuts a call's general-path queries into groups of G = min(256, budget / per-query
state) and runs k_gen_long / k_gen_short / k_gen_select (or, past limit 1,024, k_gen_compact, a
per-query sort and k_gen_write) once per group over the same dense rows, which are zeroed only when
they are made: every kernel leaves the rows it used clean for the next group, and for the next call.
These tests run more than 256 general-path queries in one call (group index >= 1, a ragged last
group, a row reused by another query within the call, the sort route's second iteration, a small
call after a large one) through every entry that reaches finish_search.

General-path queries here are those of 1..g normalised characters (g the gram size: 3 on the narrow
libraries, 2 on the wide one), which scan the whole library, and any query at a limit above 1,024.
Every test asserts the group size it relies on (the budget does not cut it below 256 on these
libraries) and the call's general_queries count, so that a change of routing or budget cannot turn
it back into a one-group test. Comparisons are exact: keys, order, fp32 bits, counts.
"""
import random

import numpy as np
import pytest
import torch

from oracle_py import OracleIndex, OracleIndexG
from test_gpu_parity import _corpus
from test_gpu_tiers import _long_queries, _short_windows
from test_gpu_wide import WIDE_ALPHA, _shape, wide_corpus

import stringsearchlib_amd as ssl

pytestmark = pytest.mark.gpu

GROUP = 256                 # kGeneralMaxGroup
BUDGET = 2 << 30            # kGeneralBudget
GUARD = 0x5A5AA5A5          # fills the output block before a call
DEV = torch.device("cuda", 0)
VALID2 = b"ABCDEFGHIJKLMabcdefghijklm0123456789 "


class Lib:
    """One index, its oracle, the key table as small integers, and the oracle's answers cached per
    (query, threshold, limit, validChar set): computed once, shared by the tests, never changed."""

    def __init__(self, gi, oi, n_words, gram, wide=False):
        self.gi, self.oi, self.n_words, self.gram, self.wide = gi, oi, n_words, gram, wide
        gi.set_timing(True)  # per-call statistics (last_stats)
        self.kid = {}
        self.canon = np.array([self.kid.setdefault(gi.key(i), len(self.kid)) for i in range(gi.num_keys())],
                              dtype=np.int64)
        self.refs = {}
        self.valid = None

    def with_index(self, gi):
        """The same library and oracle behind another index of the same words."""
        other = Lib.__new__(Lib)
        other.__dict__.update(self.__dict__)
        other.gi = gi
        gi.set_timing(True)
        assert [gi.key(i) for i in range(gi.num_keys())] == [self.gi.key(i) for i in range(self.gi.num_keys())]
        return other

    def set_valid(self, chars):
        self.gi.set_valid_char(chars)
        self.oi.set_valid_char(chars)
        self.valid = chars

    def ref(self, q, thr, limit):
        key = (q, thr, limit, self.valid)
        r = self.refs.get(key)
        if r is None:
            res = self.oi.score(q, thr, limit)
            ids = np.array([self.kid.setdefault(k, len(self.kid)) for k, _ in res], dtype=np.int64)
            bits = np.array([s for _, s in res], dtype=np.float32).view(np.uint32)
            r = self.refs[key] = (ids, bits)
        return r

    def assert_group_is_256(self):
        """ensure_general: G = min(256, 2 GiB / (4 long terms + 4 keys rounded up to 4 + 8 keys + 64));
        the terms are at most the input words, so this bound keeps G at 256 and the group borders
        at multiples of 256."""
        assert BUDGET // (16 * (self.n_words + self.gi.num_keys()) + 64) >= GROUP

    def general(self, n):
        assert self.gi.last_stats()["general_queries"] == n, self.gi.last_stats()


def _same(lib, q, ids, bits, thr, limit, where):
    rid, rbits = lib.ref(q, thr, limit)
    if len(ids) != len(rid) or not np.array_equal(ids, rid) or not np.array_equal(bits, rbits):
        bad = next((j for j in range(min(len(ids), len(rid))) if ids[j] != rid[j] or bits[j] != rbits[j]),
                   min(len(ids), len(rid)))
        raise AssertionError(f"{where} q={q!r} thr={thr} limit={limit}: {len(ids)} results vs oracle {len(rid)}, "
                             f"first difference at #{bad}: {ids[bad:bad + 3]} {bits[bad:bad + 3]} vs "
                             f"{rid[bad:bad + 3]} {rbits[bad:bad + 3]}")


def check_host(lib, qs, thr, limit, where, gi=None):
    """score_batch against the oracle; returns the call's statistics."""
    gi = gi or lib.gi
    got = gi.score_batch(qs, thr, limit)
    st = gi.last_stats()
    assert len(got) == len(qs)
    for i, (q, g) in enumerate(zip(qs, got)):
        ids = np.array([lib.kid.get(k, -1) for k, _ in g], dtype=np.int64)
        bits = np.array([s for _, s in g], dtype=np.float32).view(np.uint32)
        _same(lib, q, ids, bits, thr, limit, f"{where} #{i}")
    return st


class DeviceCall:
    """A batch in ngsSearchDevice's layout: queries on the device and an output block filled with
    a guard pattern."""

    def __init__(self, lib, qs, stride):
        self.lib, self.qs, self.stride = lib, qs, stride
        if lib.wide:
            parts = [np.array([ord(c) for c in q], dtype="<u4").tobytes() for q in qs]
        else:
            parts = list(qs)
        offs = np.zeros(len(qs) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in parts], out=offs[1:])
        self.raw = torch.frombuffer(bytearray(b"".join(parts)) or bytearray(4), dtype=torch.uint8).to(DEV)
        self.off = torch.from_numpy(offs).to(DEV)
        n = len(qs)
        self.counts = torch.full((n,), GUARD, dtype=torch.int32, device=DEV)
        self.keys = torch.full((n * stride,), GUARD, dtype=torch.int32, device=DEV)
        self.scores = torch.full((n * stride,), GUARD, dtype=torch.int32, device=DEV)

    def args(self, thr, limit):
        return (self.raw.data_ptr(), self.off.data_ptr(), len(self.qs), thr, limit, self.stride,
                self.counts.data_ptr(), self.keys.data_ptr(), self.scores.data_ptr())

    def run(self, thr, limit, stream=None):
        stream = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
        self.lib.gi.search_device(*self.args(thr, limit), stream)
        return self

    def check(self, thr, limit, where, guard=False):
        """Every query's records against the oracle; with guard, every cell past a query's count
        still holds the pattern."""
        lib, n, stride = self.lib, len(self.qs), self.stride
        c = self.counts.cpu().numpy().view(np.uint32)
        k = self.keys.cpu().numpy().view(np.uint32).reshape(n, stride)
        s = self.scores.cpu().numpy().view(np.uint32).reshape(n, stride)
        assert int(c.max(initial=0)) <= stride, f"{where}: a count of {int(c.max())} above the stride {stride}"
        nk = lib.gi.num_keys()
        for i, q in enumerate(self.qs):
            ki = k[i, :c[i]]
            assert not len(ki) or int(ki.max()) < nk, f"{where} #{i} q={q!r}: key id {int(ki.max())} of {nk} keys"
            _same(lib, q, lib.canon[ki], s[i, :c[i]], thr, limit, f"{where} #{i}")
        if guard:
            past = np.arange(stride)[None, :] >= c[:, None]
            assert bool((k[past] == GUARD).all()) and bool((s[past] == GUARD).all()), \
                f"{where}: cells past a query's count were written"


def _stride(lib, limit):
    return min(limit, lib.gi.num_keys()) if limit else lib.gi.num_keys()


def device_check(lib, qs, thr, limit, where, guard=False, stream=None):
    DeviceCall(lib, qs, _stride(lib, limit)).run(thr, limit, stream).check(thr, limit, where, guard)
    return lib.gi.last_stats()


def _norm_len(q):
    return len(q.strip(" ") if isinstance(q, str) else q.strip(b" "))


def general_queries(rng, keys, gram, n_distinct, frequent, nothing):
    """Distinct queries of 1..gram normalised characters: key prefixes, every third lower-cased, a
    few that match nothing and a few single frequent letters (they match most of the library)."""
    out = dict.fromkeys(list(frequent) + list(nothing))
    assert all(1 <= _norm_len(q) <= gram for q in out)
    pool = rng.sample(keys, min(len(keys), 8 * n_distinct))
    for i, w in enumerate(pool):
        if len(out) >= n_distinct:
            break
        q = w[:rng.randint(1, gram)]
        if i % 3 == 2:
            q = q.lower()
        if 1 <= _norm_len(q) <= gram and q != "*" and q != b"*":
            out.setdefault(q)
    assert len(out) >= n_distinct * 3 // 4, len(out)
    return list(out)


def batch(distinct, n):
    """n queries: the distinct ones over and over (their number is no divisor of 256, so a repeated
    query lands at another group position, and past 256 in another group)."""
    assert GROUP % len(distinct)
    return [distinct[i % len(distinct)] for i in range(n)]


@pytest.fixture(scope="module")
def narrow():
    words, wts, _ = ssl.synth.gen_corpus(3000, seed=31)
    lib = Lib(ssl.StringIndex(words, 1, wts), OracleIndex(words, 1, wts), len(words), 3)
    lib.words = words
    lib.weights = wts
    lib.short = general_queries(random.Random(1), words, 3, 110, [b"E", b"A", b"s"], [b"Q9X", b"9QX", b"0Q"])
    yield lib
    lib.gi.dispose()


@pytest.fixture(scope="module")
def rows():
    words, rs, wts = _corpus("rows", random.Random(13))
    lib = Lib(ssl.StringIndex(words, rs, wts), OracleIndex(words, rs, wts), len(words), 3)
    live = [w for w in words if w]
    lib.words = live
    lib.short = general_queries(random.Random(2), live, 3, 110, [b"E", b"t"], [b"Q9X", b"9Q"])
    yield lib
    lib.gi.dispose()


@pytest.fixture(scope="module")
def wide():
    rng = random.Random(3)
    words, wts = _shape(wide_corpus(rng, 2000, 1), rng)
    lib = Lib(ssl.WideStringIndex(words, 1, wts, gram_size=2), OracleIndexG(words, 1, wts, g=2, wide=True),
              len(words), 2, wide=True)
    live = [w for w in words if w and w.strip(" ")]
    lib.words = live
    assert not set("QRWqrw") & set(WIDE_ALPHA)
    lib.short = general_queries(rng, live, 2, 110, ["A", "e", "日"], ["QR", "W", "rq"])
    yield lib
    lib.gi.dispose()


@pytest.fixture
def lib(request):
    return request.getfixturevalue(request.param)


LIBS = pytest.mark.parametrize("lib", ["narrow", "rows", "wide"], indirect=True)


@LIBS
@pytest.mark.parametrize("n", [255, 256, 257, 512, 513, 700])
def test_group_borders(lib, n):
    """One group, exactly one, one query into the second, two full ones, one into the third, and a
    ragged third: k_gen_select's route at a limit that takes every scored key of most queries, a
    small one under a threshold, and the largest the select kernel takes."""
    lib.assert_group_is_256()
    qs = batch(lib.short, n)
    for thr, limit in [(0.0, 100), (0.3, 7), (0.0, 1024)]:
        st = device_check(lib, qs, thr, limit, f"borders-{n}")
        assert st["general_queries"] == n and st["queries"] == n, st


def test_interleaved_batch(narrow):
    """600 general-path queries among 600 ordinary ones (12-byte windows for tier 1a, six 70-byte
    ones for tier 2) in runs of five: a query's index is never its group position, and both group
    borders of the sorted list fall inside a run."""
    lib = narrow
    lib.assert_group_is_256()
    rng = random.Random(4)
    ordinary = _short_windows(rng, lib.words, 140) + _long_queries(rng, lib.words, 6, lo=70, hi=70)
    rng.shuffle(ordinary)
    gen = batch(lib.short, 600)
    qs, gpos = [], []
    for r in range(120):
        qs += [ordinary[(5 * r + j) % len(ordinary)] for j in range(5)]
        gpos += range(len(qs), len(qs) + 5)
        qs += gen[5 * r:5 * r + 5]
    assert len(qs) == 1200 and len(gpos) == 600
    assert all(p != i % GROUP and p != i for i, p in enumerate(gpos))
    assert gpos[256] == gpos[255] + 1 and gpos[512] == gpos[511] + 1  # the borders cut a run
    st = check_host(lib, qs, 0.3, 100, "interleaved")
    assert st["general_queries"] == 600, st
    assert st["fast_queries"] + st["general_queries"] == 1200, st
    assert st["tier2_queries"] >= 6, st
    st = device_check(lib, qs, 0.0, 100, "interleaved-device")
    assert st["general_queries"] == 600 and st["fast_queries"] == 600, st


@pytest.mark.parametrize("lib", ["narrow", "rows"], indirect=True)
@pytest.mark.parametrize("n", [300, 513])
def test_sort_route_across_groups(lib, n):
    """Past limit 1,024 every query goes general and each group ends with a host wait, a sort per
    query and k_gen_write, behind which the next group's list is queued: short queries, 12-byte
    windows and 70-byte ones (k_gen_long's counters), at limit 1,025 and at limit 0 with a stride
    of every key. The output block holds a guard pattern first; cells past a count keep it."""
    lib.assert_group_is_256()
    rng = random.Random(5)
    mix = lib.short[:40] + _short_windows(rng, lib.words, 25) + _long_queries(rng, lib.words, 4, lo=70, hi=70)
    assert len(mix) == 69
    qs = batch(mix, n)
    assert lib.gi.num_keys() > 1025
    for thr, limit in [(0.3, 1025), (0.0, 1025), (0.3, 0), (0.0, 0)]:
        st = device_check(lib, qs, thr, limit, f"sort-{n}", guard=True)
        assert st["general_queries"] == n and st["fast_queries"] == 0, st


def test_rows_left_clean_between_calls(narrow):
    """One index, call after call on the same context: the sort route, the select route over the
    same rows, a small call that uses the first ten rows only, a small limit under a threshold,
    limit 0 over half the rows, and the same batch under another validChar set."""
    words, wts = narrow.words, narrow.weights
    lib = Lib(ssl.StringIndex(words, 1, wts), OracleIndex(words, 1, wts), len(words), 3)
    lib.assert_group_is_256()
    rng = random.Random(6)
    qs = batch(narrow.short, 513)
    other = [q for q in general_queries(rng, words, 3, 60, [b"R"], [b"7QZ"]) if q not in set(narrow.short)][:10]
    assert len(other) == 10
    for step, (q, thr, limit) in enumerate([(qs, 0.0, 1025), (qs, 0.0, 100), (other, 0.0, 100), (qs, 0.5, 3),
                                            (qs[:257], 0.3, 0)]):
        st = device_check(lib, q, thr, limit, f"clean-{step}", guard=limit == 0 or limit > 1024)
        assert st["general_queries"] == len(q), (step, st)
    # another validChar set: characters outside it read as blanks, so some queries change (none
    # becomes empty: each keeps a character of the set, and stays on the general path)
    keeps = [q for q in narrow.short if any(c in VALID2 for c in q.strip())]
    assert any(any(c not in VALID2 for c in q) for q in keeps) and len(keeps) >= 60 and GROUP % len(keeps)
    qs = [keeps[i % len(keeps)] for i in range(513)]
    lib.set_valid(VALID2)
    st = device_check(lib, qs, 0.0, 100, "clean-valid")
    assert st["general_queries"] == 513, st
    st = check_host(lib, qs, 0.3, 7, "clean-valid-host")
    assert st["general_queries"] == 513, st
    lib.gi.dispose()


def test_entry_score_batch(narrow):
    narrow.assert_group_is_256()
    qs = batch(narrow.short, 513)
    for thr, limit in [(0.3, 7), (0.0, 100), (0.3, 1025)]:
        st = check_host(narrow, qs, thr, limit, "scoreBatch")
        assert st["general_queries"] == 513, st


def test_entry_search_device_on_a_side_stream(narrow):
    narrow.assert_group_is_256()
    qs = batch(narrow.short, 513)
    side = torch.cuda.Stream(DEV)
    for thr, limit in [(0.0, 100), (0.3, 1025)]:
        call = DeviceCall(narrow, qs, _stride(narrow, limit))
        side.wait_stream(torch.cuda.current_stream(DEV))  # the buffers were filled on the current stream
        call.run(thr, limit, side.cuda_stream).check(thr, limit, "side-stream", guard=limit > 1024)
        narrow.general(513)


def test_entry_async_two_batches_in_flight(narrow):
    """ngsSearchDeviceAsync twice, then the Waits in reverse order: each Wait runs its batch's
    groups on its own context while the other batch is still queued."""
    lib = narrow
    lib.assert_group_is_256()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    calls = []
    for n, thr, limit in [(513, 0.0, 100), (300, 0.3, 7)]:
        qs = batch(lib.short[n % 7:], n)
        call = DeviceCall(lib, qs, limit)
        calls.append((lib.gi.search_device_async(*call.args(thr, limit), stream), call, n, thr, limit))
    for ticket, call, n, thr, limit in reversed(calls):
        lib.gi.wait_device(ticket)
        lib.general(n)
        call.check(thr, limit, f"async-{n}")


def test_entry_split_over_two_replicas(narrow):
    """devices=[0, 0]: scoreBatch splits a batch of 8,192 (the smallest the library splits in two)
    into halves of 4,096, one per replica, each with 550 general-path queries among its windows:
    three groups on each replica's context, side by side."""
    lib = narrow
    lib.assert_group_is_256()
    gi = ssl.StringIndex(lib.words, 1, lib.weights, devices=[0, 0])
    assert gi.replicas() == 2
    two = lib.with_index(gi)
    rng = random.Random(7)
    ordinary = _short_windows(rng, lib.words, 100)
    gen = batch(lib.short, 1100)
    qs = []
    for half in range(2):
        part = [ordinary[(i + 31 * half) % len(ordinary)] for i in range(4096 - 550)]
        for j in range(550):  # a general query after every sixth window
            part.insert(7 * j + 6, gen[550 * half + j])
        assert len(part) == 4096
        qs += part
    st = check_host(two, qs, 0.3, 100, "two-replicas")
    # (the statistics are those of the slice that finished last: either half)
    assert st["queries"] == 4096 and st["general_queries"] == 550 and st["fast_queries"] == 4096 - 550, st
    gi.dispose()


def test_entry_wide_index(wide):
    wide.assert_group_is_256()
    qs = batch(wide.short, 513)
    st = check_host(wide, qs, 0.0, 100, "wide-scoreBatch")
    assert st["general_queries"] == 513, st
    st = device_check(wide, qs, 0.3, 1025, "wide-device", guard=True)
    assert st["general_queries"] == 513, st
