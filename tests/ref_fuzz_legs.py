"""The legs of the reference fuzz over an index under test (tests/test_gpu_ref_fuzz.py on the GPU,
tests/test_ref_fuzz_harness.py on the CPU with an oracle-backed index).

A stream (tests/test_ref_fuzz.py: SPECS) is loaded once: per library its words, its queries with the
thresholds drawn for them, the reference's recorded answers (tests/golden/fuzz/<name>.json) and the
oracle's answer to every (query, threshold drawn in the library, limit of the spec). The legs put those
cases to an index through a small interface, `score`, `search`, `score_batch`, `size`, `lib_size` and
`key`, and compare

* exactly with the oracle: keys, order and fp32 bits, on every case, order-dependent ones included;
* tie-aware (tiecheck.check) with the reference's recorded answer, on every case that the oracle's
  score_amb does not flag as depending on the reference's hash order, at the threshold the reference
  was asked at.
"""
from __future__ import annotations

import functools
import json
import math
import os

import test_ref_fuzz as rf
from oracle_py import OracleIndex, OracleIndexG, lib
from tiecheck import bits, check

BATCH_MIN = 17  # above the library's kSmallBatch (16): the batch path, not the latency path


class Library:
    """One library of a stream with what the reference and the oracle answer on it."""

    def __init__(self, no, words, row, weights, keys, qt, recs, limits):
        self.no, self.words, self.row, self.weights, self.keys, self.qt, self.recs = no, words, row, weights, keys, qt, recs
        self.limits = limits
        self.thresholds = []  # the distinct thresholds drawn in this library, in order
        for _, thr in qt:
            if not any(same_threshold(thr, t) for t in self.thresholds):
                self.thresholds.append(thr)
        oi = OracleIndex(words, row, weights)
        self.indexed = bool(lib().ngo_indexed(oi.h))
        self.size, self.lib_size, self.n_keys = oi.size(), oi.lib_size(), oi.n_keys()
        self.expected = {}  # (query index, threshold bits, limit) -> (answer, order-dependent in the reference)
        for qi, (q, _) in enumerate(qt):
            for thr in self.thresholds:
                for limit in limits:
                    self.expected[qi, bits(thr), limit] = oi.score_amb(q, thr, limit)
        oi.close()

    def where(self, q, thr, limit):
        return f"library {self.no} words={self.words} row={self.row} w={self.weights} q={q!r} thr={thr!r} limit={limit}"


def same_threshold(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


@functools.lru_cache(maxsize=None)
def libraries(name):
    """The libraries of stream `name`, in stream order; the recorded answers are checked to be in step."""
    spec = rf.SPECS[name]
    with open(os.path.join(rf.RECORDED, name + ".json")) as f:
        recs = iter(json.load(f)["queries"])
    out = []
    for no, (words, row, weights, keys, qt) in enumerate(rf.stream(**spec)):
        mine = [next(recs) for _ in qt]
        for (q, _), rec in zip(qt, mine):
            assert rec["q"] == q.decode("latin-1"), f"recorded case stream out of step at {q!r}"
        out.append(Library(no, words, row, weights, keys, qt, mine, spec["limits"]))
    assert next(recs, None) is None, "recorded answers past the end of the stream"
    return tuple(out)


def assert_exact(ours, ref, where):
    assert len(ours) == len(ref), f"{where}: {len(ours)} results vs oracle {len(ref)}\n{ours[:6]}\n{ref[:6]}"
    for i, ((k1, s1), (k2, s2)) in enumerate(zip(ours, ref)):
        assert k1 == k2 and bits(s1) == bits(s2), f"{where}: #{i} {k1!r}|{s1!r} vs oracle {k2!r}|{s2!r}"


class Tally:
    """What a leg did: compared cases, the ones skipped for the reference, calls per kind."""

    def __init__(self):
        self.seen = set()
        self.cases = self.vs_reference = self.order_dependent = 0
        self.singles = self.batches = self.batch_queries = self.small_batches = self.device_batches = 0

    def __str__(self):
        return (f"{len(self.seen)} libraries, {self.cases} cases exact against the oracle, {self.vs_reference} "
                f"tie-aware against the reference, {self.order_dependent} order-dependent in the reference (skipped "
                f"there), {self.singles} single calls, {self.batches} batches of {self.batch_queries} queries, "
                f"{self.small_batches} latency batches, {self.device_batches} device-API batches")


def compare(L: Library, tally: Tally, got, qi, thr, limit, oracle=True, reference=True):
    """One answer of the index under test to query qi of L at (thr, limit)."""
    q, drawn = L.qt[qi]
    where = L.where(q, thr, limit)
    exp, amb = L.expected[qi, bits(thr), limit]
    tally.cases += 1
    if oracle:
        assert_exact(got, exp, where)
    if not same_threshold(drawn, thr):
        return  # the reference was asked at the query's own threshold only
    if amb:
        tally.order_dependent += 1
        return
    if reference:
        rec = L.recs[qi]
        check(got, rec["n"][L.limits.index(limit)], [k for k, _ in rec["full"]], [b for _, b in rec["full"]], where)
        tally.vs_reference += 1


def sizes(L: Library, idx):
    assert idx.size() == L.size and idx.lib_size() == L.lib_size, \
        f"library {L.no}: size {idx.size()} / lib_size {idx.lib_size()} vs oracle {L.size} / {L.lib_size}"


def single_calls(L: Library, idx, tally: Tally, after=None, **kw):
    """score() and search() for every case of L in stream order; after() runs after every score()."""
    tally.seen.add(L.no)
    sizes(L, idx)
    for qi, (q, thr) in enumerate(L.qt):
        for limit in L.limits:
            got = idx.score(q, thr, limit)
            tally.singles += 1
            if after:
                after()
            compare(L, tally, got, qi, thr, limit, **kw)
            assert idx.search(q, thr, limit) == [k for k, _ in got], f"{L.where(q, thr, limit)}: search() != score()"


def batches(L: Library, idx, tally: Tally, small=True, after=None, device=None, **kw):
    """score_batch at every threshold drawn in L and every limit over L's queries, repeated to at least
    BATCH_MIN; then (small) the first 16 of them as a latency batch, and (device) the same batch through
    device(idx, queries, thr, limit). after(n) runs after every batch of n > 16 queries."""
    tally.seen.add(L.no)
    sizes(L, idx)
    qs = [q for q, _ in L.qt]
    n = len(qs)
    batch = qs * -(-BATCH_MIN // n)
    assert len(batch) >= BATCH_MIN
    for thr in L.thresholds:
        for limit in L.limits:
            got = idx.score_batch(batch, thr, limit)
            tally.batches += 1
            tally.batch_queries += len(batch)
            if after:
                after(len(batch))
            assert len(got) == len(batch)
            for i, g in enumerate(got):
                if i < n:
                    compare(L, tally, g, i, thr, limit, **kw)
                else:
                    assert_exact(g, got[i % n], f"{L.where(batch[i], thr, limit)}: copy #{i // n} vs the first")
            if device:
                for i, g in enumerate(device(idx, batch, thr, limit)):
                    assert_exact(g, got[i], f"{L.where(batch[i], thr, limit)}: device API vs host batch")
                tally.device_batches += 1
            if small:  # (last: the next batch's after() then follows a call of at most 16 queries)
                few = batch[:16]
                for i, g in enumerate(idx.score_batch(few, thr, limit)):
                    assert_exact(g, got[i], f"{L.where(few[i], thr, limit)}: latency batch vs batch")
                tally.small_batches += 1


def against(L: Library, idx, ref, tally: Tally, after=None):
    """Single calls and batches of L's cases on idx, exact against another index `ref` of the same
    interface (the gram sizes the reference does not have: no recorded answers)."""
    tally.seen.add(L.no)
    assert idx.size() == ref.size() and idx.lib_size() == ref.lib_size(), f"library {L.no}: sizes"
    for q, thr in L.qt:
        for limit in L.limits:
            got = idx.score(q, thr, limit)
            tally.singles += 1
            tally.cases += 1
            assert_exact(got, ref.score(q, thr, limit), L.where(q, thr, limit))
            assert idx.search(q, thr, limit) == [k for k, _ in got], f"{L.where(q, thr, limit)}: search() != score()"
    qs = [q for q, _ in L.qt]
    batch = qs * -(-BATCH_MIN // len(qs))
    for thr in L.thresholds:
        for limit in L.limits:
            got = idx.score_batch(batch, thr, limit)
            tally.batches += 1
            tally.batch_queries += len(batch)
            if after:
                after(len(batch))
            for q, g in zip(batch, got):
                tally.cases += 1
                assert_exact(g, ref.score(q, thr, limit), f"{L.where(q, thr, limit)}: batch")


class Decoded:
    """A wide or UTF-8 index behind the byte-string interface (ASCII streams: one unit per byte)."""

    def __init__(self, idx):
        self.idx = idx

    @staticmethod
    def _out(res):
        return [(k.encode("latin-1"), s) for k, s in res]

    def score(self, q, thr, limit):
        return self._out(self.idx.score(q.decode("latin-1"), thr, limit))

    def search(self, q, thr, limit):
        return [k.encode("latin-1") for k in self.idx.search(q.decode("latin-1"), thr, limit)]

    def score_batch(self, qs, thr, limit):
        return [self._out(r) for r in self.idx.score_batch([q.decode("latin-1") for q in qs], thr, limit)]

    def size(self):
        return self.idx.size()

    def lib_size(self):
        return self.idx.lib_size()

    def key(self, k):
        return self.idx.key(k).encode("latin-1")


class OracleBacked:
    """The interface over the oracle itself (g = 3: OracleIndex; else OracleIndexG): what a correct
    index answers. tests/test_ref_fuzz_harness.py derives deliberately wrong ones from it."""

    def __init__(self, words, row, weights, g=3):
        self.oi = OracleIndex(words, row, weights) if g == 3 else OracleIndexG(words, row, weights, g=g)

    def score(self, q, thr, limit):
        return self.oi.score(q, thr, limit)

    def search(self, q, thr, limit):
        return [k for k, _ in self.score(q, thr, limit)]

    def score_batch(self, qs, thr, limit):
        return [self.score(q, thr, limit) for q in qs]

    def size(self):
        return self.oi.size()

    def lib_size(self):
        return self.oi.lib_size()

    def key(self, k):
        return self.oi.key(k)

    def dispose(self):
        self.oi.close()
