"""The CPU restatement against the REFERENCE itself on random corpora with large weights (CPU).

The reference (nGramSearch/dllmain.cpp) and oracle/ngs_oracle.c answer the same seeded cases; the
answers are compared tie-aware (tests/tiecheck.py). The reference's answers to every case are
recorded under tests/golden/fuzz/ (tests/golden/make_golden_fuzz.py writes them), so the fuzz runs
wherever the suite does; where oracle/Makefile has compiled the reference into oracle/_ref/, the
same cases are also put to the compiled reference itself. Weights come from {1, 100, 150, 1000, 0, -1}
(plus 0.5 and 2), so scores w*s above, at and below the promotion score 100 meet promoted keys
(nGramSearch.hpp:326-337): a promoted key is the score 100 in ScoreComparer
(nGramSearch.h:262-269), so a key with w*s = 150 ranks above it and one at exactly 100 ties
with it and is ordered by length. Queries are mostly keys themselves, lower-cased keys and
pieces of keys, at limits 1, 3, 100 and 0 (unlimited) and thresholds 0, 0.3 and 0.5.

Cases whose reference answer depends on unordered_map iteration order beyond (score, length)
ties — a promoted key with another pair above 100 in the same calcScore pass — are counted
and skipped (ngo_search_amb decides; ngs_oracle.c header). The wildcard queries "" / "*",
whose multi-pair keys take "the last pair in hash order" (hpp:356-369), are not drawn here.

A third stream, HOSTILE (recorded as hostile_inputs), puts the inputs to the reference that the two
above leave out: bytes >= 0x80 (outside validChar, so escapeBlank turns them into blanks, and the gram
hash runs over signed chars, nGramSearch.h:147-150), punctuation and tabs, NULL alias words inside
tiny rows, alias words that several rows share, libraries of one or two words, terms of 60-80 characters (58-78 grams), FLT_MAX and
subnormal weights next to normal ones, and libraries with the single weight 200 or 200.00002 (either
side of the library's rank-list rule). Weights of +-inf are NOT drawn, like NaN weights: a short-search
score of 0 gives inf * 0 = NaN in calcScore (hpp:326; std::max keeps a NaN first argument), and a NaN
score has no order in ScoreComparer, so the reference's answer to such a case is whatever its sort leaves. Queries that are
"" or "*" or blank once normalised are not drawn either.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import random

from oracle_py import OracleIndex
from tiecheck import bits, check, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libStringSearchLib.so")
RECORDED = os.path.join(ROOT, "tests", "golden", "fuzz")
WEIGHTS = [1.0, 100.0, 150.0, 1000.0, 0.0, -1.0, 0.5, 2.0]


class LiveReference:
    """The compiled reference (oracle/_ref/libStringSearchLib.so) through its C ABI."""

    def __init__(self):
        L = C.CDLL(REF_SO)
        L.indexN.restype = C.c_uint32
        L.indexN.argtypes = [C.POINTER(C.c_char_p), C.c_uint64, C.c_uint16, C.POINTER(C.c_float)]
        L.score.restype = C.c_uint32
        L.score.argtypes = [C.c_uint32, C.c_char_p, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_float)),
                            C.c_float, C.c_uint32]
        L.release.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_float)]
        L.dispose.argtypes = [C.c_uint32]
        self.L, self.h = L, 0

    def open(self, words, row, weights):
        wa = (C.c_char_p * len(words))(*words)
        wf = (C.c_float * len(weights))(*weights)
        self.h = self.L.indexN(wa, len(words), row, wf)
        assert self.h

    def score(self, q: bytes, thr: float, limit: int):
        res = C.POINTER(C.c_char_p)()
        sc = C.POINTER(C.c_float)()
        n = self.L.score(self.h, q, C.byref(res), C.byref(sc), thr, limit)
        out = [(res[i], sc[i]) for i in range(n)]
        self.L.release(self.h, res, sc)
        return out

    def full(self, q, thr, limits):
        return self.score(q, thr, 0)

    def count(self, q, thr, limit):
        return len(self.score(q, thr, limit))

    def close(self):
        self.L.dispose(self.h)


class RecordingReference(LiveReference):
    """The compiled reference, keeping what it answered: per query its full (limit 0) answer and
    the number of results at every limit of the case (tests/golden/make_golden_fuzz.py)."""

    def __init__(self):
        super().__init__()
        self.queries = []

    def full(self, q, thr, limits):
        out = self.score(q, thr, 0)
        self.queries.append({"q": q.decode("latin-1"), "full": [[k.decode("latin-1"), bits(s)] for k, s in out],
                             "n": [len(out) if lim == 0 else len(self.score(q, thr, lim)) for lim in limits]})
        return out


class RecordedReference:
    """The reference's recorded answers (tests/golden/fuzz/<name>.json), read back in case order."""

    def __init__(self, name):
        with open(os.path.join(RECORDED, name + ".json")) as f:
            self.queries = iter(json.load(f)["queries"])
        self.rec = self.limits = None

    def open(self, words, row, weights):
        pass

    def full(self, q, thr, limits):
        self.rec, self.limits = next(self.queries), limits
        assert self.rec["q"] == q.decode("latin-1"), f"recorded case stream out of step at {q!r}"
        return [(k.encode("latin-1"), f32(b)) for k, b in self.rec["full"]]

    def count(self, q, thr, limit):
        return self.rec["n"][self.limits.index(limit)]

    def close(self):
        pass


def references(name):
    """The recorded answers, and the compiled reference where it was built."""
    return [RecordedReference(name)] + ([LiveReference()] if os.path.exists(REF_SO) else [])


def _corpus(rng: random.Random):
    alpha = "ABCDE" if rng.random() < 0.5 else "ABCDEFGH XY"
    row = rng.choice([1, 1, 2, 3])
    n_rows = rng.randint(3, 14)
    words, weights = [], []
    keys = []
    for _ in range(n_rows):
        for j in range(row):
            r = rng.random()
            if j == 0 and keys and r < 0.15:
                w = rng.choice(keys)                      # a repeated key: more pairs for one key
            elif r < 0.25:
                w = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 5)))   # short term
            else:
                w = "".join(rng.choice(alpha) for _ in range(rng.randint(6, 12)))  # long term
            if rng.random() < 0.15:
                w = w.lower()
            if j == 0:
                keys.append(w)
            words.append(w.encode())
            weights.append(rng.choice(WEIGHTS))
    return words, row, weights, keys


def _queries(rng: random.Random, words, keys, n):
    out = []
    for _ in range(n):
        r = rng.random()
        src = rng.choice(keys).encode()
        if r < 0.45:
            q = src                                        # an exact key: promotion
        elif r < 0.55:
            q = src.lower()
        elif r < 0.8:
            w = rng.choice(words)
            a = rng.randrange(len(w))
            q = w[a:a + rng.randint(1, 9)]                 # a piece: short and long searches
        else:
            w = bytearray(rng.choice(words))
            w[rng.randrange(len(w))] = ord(rng.choice("ABCDEXYZ"))
            q = bytes(w)
        if q in (b"", b"*"):
            q = b"A"
        out.append(q)
    return out


def stream(seed, n_cases, n_queries, thresholds, limits, corpus, queries):
    """The case stream of a spec, one library at a time: (words, row, weights, keys, [(query, threshold)]).
    The rng is drawn from in a fixed order (the library, its queries, then one threshold per query), so
    every consumer of a spec (fuzz() here, the recorder, tests/test_gpu_ref_fuzz.py) sees the same cases
    as the recorded answers; a case is one (query, threshold) at one of the spec's limits."""
    rng = random.Random(seed)
    cases = 0
    while cases < n_cases:
        words, row, weights, keys = corpus(rng)
        qt = [(q, rng.choice(thresholds)) for q in queries(rng, words, keys, n_queries)]
        yield words, row, weights, keys, qt
        cases += len(qt) * len(limits)


def fuzz(ref, **spec):
    """Puts the seeded cases to `ref` and to the oracle; (cases, order-dependent cases, failures)."""
    limits = spec["limits"]
    cases = ambiguous = 0
    failures = []
    for words, row, weights, keys, qt in stream(**spec):
        ref.open(words, row, weights)
        oi = OracleIndex(words, row, weights)
        for q, thr in qt:
            full = ref.full(q, thr, limits)
            for limit in limits:
                cases += 1
                ours, amb = oi.score_amb(q, thr, limit)
                if amb:
                    ambiguous += 1
                    continue
                n_ref = len(full) if limit == 0 else ref.count(q, thr, limit)
                if limit >= 2**31:
                    assert n_ref == len(full), (q, thr, limit)
                try:
                    check(ours, n_ref, [k for k, _ in full], [bits(s) for _, s in full],
                          f"words={words} row={row} w={weights} q={q!r} thr={thr} limit={limit}")
                except AssertionError as e:
                    failures.append(str(e))
        ref.close()
        oi.close()
    return cases, ambiguous, failures


LARGE_WEIGHTS = dict(seed=20261018, n_cases=6000, n_queries=12, thresholds=[0.0, 0.0, 0.3, 0.5],
                     limits=[1, 3, 100, 0], corpus=_corpus, queries=_queries)


def test_oracle_vs_reference_large_weights():
    for ref in references("large_weights"):
        cases, ambiguous, failures = fuzz(ref, **LARGE_WEIGHTS)
        print(f"{type(ref).__name__}: {cases} cases, {ambiguous} order-dependent in the reference (skipped), "
              f"{len(failures)} failures")
        assert not failures, f"{len(failures)} of {cases} cases differ; first: {failures[0]}"
        assert ambiguous < cases // 10


# thresholds outside [0, 1], NaN and near 1, limits past 2^31 (VERDICT r5 ask 3): the reference tests
# `s < threshold` as written (nGramSearch.hpp:315), so NaN and negative thresholds skip nothing and
# thresholds above 1 keep only the short-search and promoted pairs that reach them; `limit` is a
# uint32 taken as given (hpp:399-401, 420-425), 0 meaning every result
DEGENERATE_THRESHOLDS = [-1.0, float("nan"), 1.0, 1.5, 0.999, 1.0 / 3.0, 2.0 / 3.0, 0.7]
DEGENERATE_LIMITS = [1, 2**31, 2**32 - 1, 0]
DEGENERATE = dict(seed=61018, n_cases=2000, n_queries=8, thresholds=DEGENERATE_THRESHOLDS,
                  limits=DEGENERATE_LIMITS, corpus=_corpus, queries=_queries)


def test_oracle_vs_reference_degenerate_args():
    for ref in references("degenerate_args"):
        cases, ambiguous, failures = fuzz(ref, **DEGENERATE)
        print(f"{type(ref).__name__}: {cases} cases, {ambiguous} order-dependent in the reference (skipped), "
              f"{len(failures)} failures")
        assert not failures, f"{len(failures)} of {cases} cases differ; first: {failures[0]}"
        assert ambiguous < cases // 10


# ---- the hostile stream: the inputs the two streams above leave out (module docstring) ----
FLT_MAX = 3.4028234663852886e38
HOSTILE_ALPHABETS = [b"ABCDE\xe9\xff\x80", b"ABCab \t.-_#", b"ABC"]
# 1e-45 and 1e-38 are subnormal in fp32 (flushing them to zero would change bits); 200 and 200.00002
# (fp32 0x43480001) sit either side of the library's rank-list rule w <= 200
HOSTILE_WEIGHTS = [1.0, 100.0, 150.0, 0.0, -1.0, 0.5, FLT_MAX, 1e-45, 1e-38, 200.0, 200.00002]
HOSTILE_ONE_WEIGHT = [1.0, 200.0, 200.00002, -1.0, 1e-45, 0.5, 2.5]
_VALID = set(b".%$ @0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")  # nGramSearch.h:307-313


def _normal(w: bytes) -> bytes:
    """escapeBlank, trim, toUpper (nGramSearch.h:30-98) under the default validChar: the term of a word."""
    return bytes(c if c in _VALID else 32 for c in w).strip(b" \t\n\v\f\r").upper()


def _hostile_word(rng: random.Random, alpha: bytes) -> bytes:
    r = rng.random()
    n = rng.randint(1, 5) if r < 0.2 else rng.randint(6, 12) if r < 0.9 else rng.randint(60, 80)
    return bytes(rng.choice(alpha) for _ in range(n))


def _hostile_corpus(rng: random.Random):
    alpha = rng.choice(HOSTILE_ALPHABETS)
    n_rows = rng.randint(1, 14)
    words, weights, keys = [], [], []
    if rng.random() < 0.2:
        # a one-weight library of distinct terms, one per key: unique keys and one pair per term, so
        # the weight alone decides whether the library takes rank lists
        w1 = rng.choice(HOSTILE_ONE_WEIGHT)
        seen = set()
        for _ in range(n_rows):
            w = _hostile_word(rng, alpha)
            if _normal(w) in seen or not _normal(w):
                continue
            seen.add(_normal(w))
            keys.append(w)
        if not keys:
            keys.append(b"ABCABCA")
        return list(keys), 1, [w1] * len(keys), keys
    row = rng.choice([1, 1, 2, 3])
    for _ in range(n_rows):
        for j in range(row):
            if j == 0 and keys and rng.random() < 0.15:
                w = rng.choice(keys)                      # a repeated key: more pairs for one key
            elif j and rng.random() < 0.1:
                w = None                                  # a NULL alias word (hpp:150-157 skips it)
            elif j and rng.random() < 0.15:
                w = rng.choice([x for x in words if x])   # an alias other rows have: a term of several keys
            else:
                w = _hostile_word(rng, alpha)
            if j == 0:
                keys.append(w)
            words.append(w)
            weights.append(rng.choice(HOSTILE_WEIGHTS))
    return words, row, weights, keys


def _hostile_queries(rng: random.Random, words, keys, n):
    real = [w for w in words if w]
    out = []
    for _ in range(n):
        r = rng.random()
        src = rng.choice(keys)
        if r < 0.4:
            q = src                                        # an exact key: promotion
        elif r < 0.5:
            q = src.lower()
        elif r < 0.8:
            w = rng.choice(real)
            a = rng.randrange(len(w))
            q = w[a:a + rng.randint(1, 9)]                 # a piece: short and long searches
        else:
            w = bytearray(rng.choice(real))
            w[rng.randrange(len(w))] = rng.choice(b"ABCXYZ\xe9 ")
            q = bytes(w)
        if not _normal(q) or q.strip() == b"*":            # the wildcard, or blank once normalised
            q = b"A"
        out.append(q)
    return out


HOSTILE = dict(seed=20261019, n_cases=4000, n_queries=12, thresholds=[0.0, 0.3, 0.5, 1.0], limits=[1, 3, 100, 0],
               corpus=_hostile_corpus, queries=_hostile_queries)
SPECS = {"large_weights": LARGE_WEIGHTS, "degenerate_args": DEGENERATE, "hostile_inputs": HOSTILE}


def test_oracle_vs_reference_hostile_inputs():
    for ref in references("hostile_inputs"):
        cases, ambiguous, failures = fuzz(ref, **HOSTILE)
        print(f"{type(ref).__name__}: {cases} cases, {ambiguous} order-dependent in the reference (skipped), "
              f"{len(failures)} failures")
        assert not failures, f"{len(failures)} of {cases} cases differ; first: {failures[0]}"
        assert ambiguous < cases // 10
