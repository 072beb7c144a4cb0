"""The reference fuzz on the GPU: every tiny library of tests/test_ref_fuzz.py through every entry point.

The three recorded streams (large_weights, degenerate_args, hostile_inputs) hold some 400 libraries of
at most 42 words: the small end of kernels dimensioned for millions of rows, where L = min(limit, keys)
is below one wave, there is one skip bucket, heavy_slices is clamped to the bucket count, the long or
the short library is empty, and keys_unique, tk_identity, tk_monotone and the rank lists flip from one
library to the next. Every answer is compared exactly with the oracle (keys, order, fp32 bits), and
every case the oracle does not flag as order-dependent in the reference also tie-aware with the
reference's recorded answer (tests/ref_fuzz_legs.py; tests/test_ref_fuzz_harness.py shows on the CPU
that these legs catch a dropped result, a one-ulp score and a swapped tie).

Legs, one test per (stream, leg):
* default   score()/search() per case on a handle left at its serve preference: the first calls take
            the latency path, later ones the server kernel once it starts by itself (the library has
            one skip bucket); at least one library per stream must have reached serve_state() == 2;
* latency   the same calls after serve(False): serve_state() stays 0;
* batch     score_batch over the library's queries repeated to >= 17 (above kSmallBatch) at every
            threshold drawn in the library and every limit, its first 16 again as a latency batch, and
            the same bytes through search_device; last_stats() must show each batch above 16 queries;
* build     (hostile_inputs) the device build's ngsIndexDigest equals both host builds'
            (NGS_HOST_INTERN=1, NGS_HOST_GRAMS=1); over the stream each shape flag of digest word 16
            (1 keys unique, 2 one pair per term, 4 term ids in key-rank order, 8 rank lists) must be
            seen set and clear at least five times;
* wide, utf8  (the two ASCII streams) WideStringIndex / Utf8StringIndex at gram size 3 answer like the
            narrow oracle and the recorded reference; not run on hostile_inputs, where a wide index
            does hit grams with code points 0x80-0xFF, unlike the reference's signed-char hash;
* g1, g2    (large_weights) StringIndex(gram_size=g) exactly like OracleIndexG(g=g).

The narrow legs run every library. The secondary legs (build, wide, utf8, g1, g2) take every
K_SECONDARY-th library; K_SECONDARY = 1 takes all of them.
"""
import ctypes as C
import functools
import os
import time

import pytest

import ref_fuzz_legs as legs
import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

pytestmark = pytest.mark.gpu

K_SECONDARY = 1
STREAMS = list(legs.rf.SPECS)
ASCII_STREAMS = ["large_weights", "degenerate_args"]
FLAGS = {1: "keys_unique", 2: "tk_identity", 4: "tk_monotone", 8: "rank lists"}


class Builds:
    """Index constructors, timed."""

    def __init__(self):
        self.ms = []

    def __call__(self, cls, *args, env=None, **kw):
        if env:
            os.environ[env] = "1"
        t0 = time.perf_counter()
        try:
            idx = cls(*args, **kw)
        finally:
            if env:
                os.environ.pop(env, None)
        self.ms.append((time.perf_counter() - t0) * 1e3)
        return idx

    def __str__(self):
        ms = sorted(self.ms)
        return f"{len(ms)} builds, median {ms[len(ms) // 2]:.2f} ms, mean {sum(ms) / len(ms):.2f} ms, max {ms[-1]:.2f} ms"


def _summary(name, leg, tally, builds, extra=""):
    print(f"{name}/{leg}: {tally}; {builds}{extra}")


def _batch_stats(gi, seen, indexed, n):
    """After a host batch of n > 16 queries: the call's statistics must be a batch's, not a latency call's."""
    if not indexed:  # fewer than two words: no index, nothing is launched (nGramSearch.hpp:122-123, 417-418)
        return
    st = gi.last_stats()
    assert st["queries"] == n > 16, f"last_stats() after a batch of {n}: {st['queries']} queries"
    seen.append(n)


def _device_batch(indexed, idx, qs, thr, limit):
    """search_device over the raw bytes and offsets of qs; ids mapped to keys with key()."""
    import torch
    dev = torch.device("cuda:0")
    raw = torch.frombuffer(bytearray(b"".join(qs)), dtype=torch.uint8).to(dev)
    offs = [0]
    for q in qs:
        offs.append(offs[-1] + len(q))
    off = torch.tensor(offs, dtype=torch.int64, device=dev)
    stride = max(1, min(limit or 2**31 - 1, idx.num_keys()))
    counts = torch.full((len(qs),), -1, dtype=torch.int32, device=dev)
    keys = torch.zeros(len(qs) * stride, dtype=torch.int32, device=dev)
    scores = torch.zeros(len(qs) * stride, dtype=torch.float32, device=dev)
    args = (raw.data_ptr(), off.data_ptr(), len(qs), thr, limit, stride, counts.data_ptr(), keys.data_ptr(),
            scores.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if not indexed:  # a library of fewer than two words is not built (nGramSearch.hpp:122-123): refused (-2)
        with pytest.raises(RuntimeError):
            idx.search_device(*args)
        return [[] for _ in qs]
    idx.search_device(*args)
    torch.cuda.synchronize()
    c, k, s = counts.cpu().tolist(), keys.cpu().tolist(), scores.cpu().tolist()
    assert all(0 <= n <= stride for n in c), f"device counts {c} (stride {stride})"
    return [[(idx.key(k[i * stride + j]), s[i * stride + j]) for j in range(c[i])] for i in range(len(qs))]


@pytest.mark.parametrize("name", STREAMS)
def test_single_calls_default_preference(name):
    tally, builds = legs.Tally(), Builds()
    served_calls, served_libraries = [0], 0
    for L in legs.libraries(name):
        gi = builds(ssl.StringIndex, L.words, L.row, L.weights)
        before = served_calls[0]

        def after():
            served_calls[0] += gi.serve_state() == 2
        try:
            legs.single_calls(L, gi, tally, after=after)
        finally:
            gi.dispose()
        served_libraries += served_calls[0] > before
    _summary(name, "default", tally, builds, f"; {served_calls[0]} calls left the server kernel running, in "
                                             f"{served_libraries} libraries; {tally.singles - served_calls[0]} did not")
    assert served_libraries >= 1, "no library reached serve_state() == 2: the server never started by itself"
    assert tally.singles > served_calls[0] > 0


@pytest.mark.parametrize("name", STREAMS)
def test_single_calls_latency_path(name):
    tally, builds = legs.Tally(), Builds()
    for L in legs.libraries(name):
        gi = builds(ssl.StringIndex, L.words, L.row, L.weights)

        def after():
            assert gi.serve_state() == 0, f"library {L.no}: a server after serve(False)"
        try:
            if L.indexed:
                gi.serve(False)
            else:  # fewer than two words: no index (nGramSearch.hpp:122-123), nothing to serve (-2)
                with pytest.raises(RuntimeError):
                    gi.serve(False)
            legs.single_calls(L, gi, tally, after=after)
        finally:
            gi.dispose()
    _summary(name, "latency", tally, builds)
    assert tally.singles == sum(len(L.qt) for L in legs.libraries(name)) * len(legs.rf.SPECS[name]["limits"])


@pytest.mark.parametrize("name", STREAMS)
def test_batches_latency_batches_and_device_api(name):
    pytest.importorskip("torch")
    tally, builds, seen = legs.Tally(), Builds(), []
    for L in legs.libraries(name):
        gi = builds(ssl.StringIndex, L.words, L.row, L.weights)
        try:
            gi.set_timing(True)  # last_stats() is filled only then
            legs.batches(L, gi, tally, after=functools.partial(_batch_stats, gi, seen, L.indexed),
                         device=functools.partial(_device_batch, L.indexed))
        finally:
            gi.dispose()
    _summary(name, "batch", tally, builds)
    assert tally.batches >= len(seen) > tally.batches * 3 // 4 and min(seen) >= legs.BATCH_MIN
    assert tally.small_batches == tally.device_batches == tally.batches


def _digest(idx, indexed=True):
    out = (C.c_uint64 * 17)()
    rc = _native.lib().ngsIndexDigest(idx.handle, out, 17)
    assert rc == (17 if indexed else -1)  # (no index, no replica to digest: fewer than two words)
    return list(out) if indexed else None


def test_device_build_matches_host_builds_and_covers_the_shape_flags():
    name = "hostile_inputs"
    builds = Builds()
    flags, predicted = [], 0
    for L in legs.libraries(name)[::K_SECONDARY]:
        g = builds(ssl.StringIndex, L.words, L.row, L.weights)
        hi = builds(ssl.StringIndex, L.words, L.row, L.weights, env="NGS_HOST_INTERN")
        hg = builds(ssl.StringIndex, L.words, L.row, L.weights, env="NGS_HOST_GRAMS")
        try:
            dg = _digest(g, L.indexed)
            assert dg == _digest(hi, L.indexed), f"library {L.no} words={L.words} row={L.row} w={L.weights}: device build vs host intern"
            assert dg == _digest(hg, L.indexed), f"library {L.no} words={L.words} row={L.row} w={L.weights}: device build vs host grams"
            for idx in (g, hi, hg):
                legs.sizes(L, idx)
            if not L.indexed:
                continue
            flags.append(dg[16])
            # what the construction decides: rows of one word, every word another term, one weight ->
            # unique keys, one pair per term, and rank lists exactly when the weight is at most 200
            terms = [legs.rf._normal(w) for w in L.words] if L.row == 1 else []
            if terms and all(terms) and len(set(terms)) == len(terms) and len(set(L.weights)) == 1 \
                    and L.weights[0] != 0.0:
                want = 3 | (8 if L.weights[0] <= 200.0 else 0)
                assert dg[16] & 11 == want, f"library {L.no} w={L.weights[0]!r}: flags {dg[16]:#x}, expected {want:#x}"
                predicted += 1
        finally:
            for idx in (g, hi, hg):
                idx.dispose()
    seen = {bit: (sum(1 for f in flags if f & bit), sum(1 for f in flags if not f & bit)) for bit in FLAGS}
    print(f"{name}/build: {len(flags)} libraries, flags predicted for {predicted}; {builds}; flags set/clear: "
          + ", ".join(f"{FLAGS[b]} {s}/{c}" for b, (s, c) in seen.items()))
    for bit, (s, c) in seen.items():
        assert s >= 5 and c >= 5, f"{FLAGS[bit]}: set in {s} libraries, clear in {c}"


def _decoded(words):
    return [None if w is None else w.decode("latin-1") for w in words]


@pytest.mark.parametrize("cls", [ssl.WideStringIndex, ssl.Utf8StringIndex], ids=["wide", "utf8"])
@pytest.mark.parametrize("name", ASCII_STREAMS)
def test_wide_and_utf8_front_ends(name, cls):
    tally, builds, seen = legs.Tally(), Builds(), []
    for L in legs.libraries(name)[::K_SECONDARY]:
        gi = builds(cls, _decoded(L.words), L.row, L.weights, gram_size=3)
        try:
            gi.set_timing(True)
            idx = legs.Decoded(gi)
            legs.single_calls(L, idx, tally)
            legs.batches(L, idx, tally, small=False, after=functools.partial(_batch_stats, gi, seen, L.indexed))
        finally:
            gi.dispose()
    _summary(name, cls.__name__, tally, builds)
    assert tally.batches >= len(seen) > tally.batches * 3 // 4 and tally.singles > 0 and tally.vs_reference > 0


@pytest.mark.parametrize("g", [1, 2])
def test_gram_sizes_1_and_2(g):
    name = "large_weights"
    tally, builds, seen = legs.Tally(), Builds(), []
    for L in legs.libraries(name)[::K_SECONDARY]:
        gi = builds(ssl.StringIndex, L.words, L.row, L.weights, gram_size=g)
        ref = legs.OracleBacked(L.words, L.row, L.weights, g=g)
        try:
            gi.set_timing(True)
            legs.against(L, gi, ref, tally, after=functools.partial(_batch_stats, gi, seen, L.indexed))
        finally:
            gi.dispose()
            ref.dispose()
    _summary(name, f"g{g}", tally, builds)
    assert tally.batches >= len(seen) > tally.batches * 3 // 4 and tally.singles > 0
