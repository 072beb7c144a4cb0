"""The libraries and query batches of the index-set GPU tests (tests/test_gpu_set.py), built from the
synthetic corpus helpers; the host test checks on the CPU that the oracle flags none of the narrow
queries as ambiguous (tests/test_set_host.py)."""
from __future__ import annotations

import functools
import random

import stringsearchlib_amd as ssl

ROW = 2                      # master key plus alias
THRESHOLDS = (0.0, 0.3)
LIMITS = (1, 10, 100, 0)
TIE_QUERY = b"QJXQKZVQWJ"    # the family's common head: every family key scores alike for it
FAMILY = 300


@functools.lru_cache(maxsize=None)
def narrow():
    """(words, weights, cuts): 6,000 rows of (master key, alias) with per-word weights, master keys unique;
    300 rows spread over the library are the tie family (one length, one weight, the query's head and a
    tail of digits no other gram shares). cuts: the row boundaries of 3 uneven parts, the first of 2 rows."""
    rows = 6000
    words, weights, _ = ssl.synth.gen_corpus(rows, seed=77, min_len=6, span=14, row_size=ROW)
    words, weights = list(words), list(weights)
    rng = random.Random(77)
    for n, r in enumerate(sorted(rng.sample(range(2, rows), FAMILY))):
        words[ROW * r] = TIE_QUERY + b"%03d" % n
        words[ROW * r + 1] = b"Z%05dY" % n
        weights[ROW * r] = weights[ROW * r + 1] = 1.0
    masters = words[::ROW]
    assert len(set(masters)) == rows
    return words, weights, (0, 2, 2500, rows)


@functools.lru_cache(maxsize=None)
def narrow_queries():
    """About 200 queries: ordinary ones, "" and "*", 1-3 characters (the whole-library scan), exact
    matches whose key lies in the last part (promoted to 100), the tie family's."""
    words, _, cuts = narrow()
    rng = ssl.synth.SplitMix64(5)
    qs = ssl.synth.gen_queries(words, ROW, 150, rng)
    qs += [b"", b"*", b"A", b"Q", b"7", b"AB", b"QJ", b"Z0", b"ABC", b"QJX", b"XQK", b"00Y", b"E R"]
    last = words[ROW * cuts[2]::ROW]
    qs += [last[i] for i in range(0, len(last), len(last) // 24)][:24]
    qs += [last[7].lower(), words[0], words[ROW]]          # (the first part's two keys too)
    qs += [TIE_QUERY, TIE_QUERY + b"0", TIE_QUERY[:7], TIE_QUERY + b"299", b"Z00017Y"]
    return qs


def split(words, weights, cuts):
    """[(words, weights)] of the contiguous row ranges."""
    return [(words[ROW * a:ROW * b], weights[ROW * a:ROW * b]) for a, b in zip(cuts, cuts[1:])]


WIDE_TIE_QUERY = "жQéKZ漢VW"  # the wide family's common head
WIDE_FAMILY = 130               # more than the largest limit: limits 10 and 100 fall inside the tie class
SPICE = {"A": "é", "K": "ж", "7": "漢", "Q": "\U0001f600"}  # 2-, 2-, 3- and 4-byte UTF-8


@functools.lru_cache(maxsize=None)
def wide():
    """(words as str, weights, cuts): 1,500 rows of (master key, alias), some letters replaced by
    characters of 2 to 4 UTF-8 bytes; 130 rows spread over the library are the tie family, as in narrow();
    2 parts."""
    rows = 1500
    words, weights, _ = ssl.synth.gen_corpus(rows, seed=78, min_len=4, span=10, row_size=ROW)
    out = []
    for i, w in enumerate(words):
        s = w.decode("latin-1")
        if i % 3 == 0:
            s = "".join(SPICE.get(c, c) for c in s)
        out.append(s)
    weights = list(weights)
    rng = random.Random(79)
    for n, r in enumerate(sorted(rng.sample(range(rows), WIDE_FAMILY))):
        out[ROW * r] = WIDE_TIE_QUERY + "%03d" % n
        out[ROW * r + 1] = "Z%05dY" % n
        weights[ROW * r] = weights[ROW * r + 1] = 1.0
    assert len(set(out[::ROW])) == rows
    return out, weights, (0, 611, rows)


@functools.lru_cache(maxsize=None)
def wide_queries():
    words, _, cuts = wide()
    rng = random.Random(78)
    qs = []
    for _ in range(40):
        w = rng.choice(words[::ROW])
        o = rng.randrange(0, max(1, len(w) - 5))
        q = list(w[o:o + 8])
        q[rng.randrange(len(q))] = rng.choice("BCDEFé漢")
        qs.append("".join(q))
    qs += ["", "*", "é", "B", "7", "ж漢", "Z0", "QéK", "00Y", words[0]]
    last = words[ROW * cuts[1]::ROW]
    qs += [last[i] for i in range(0, len(last), len(last) // 12)][:12] + [last[-1]]  # promoted, in the last part
    qs += [WIDE_TIE_QUERY, WIDE_TIE_QUERY + "0", WIDE_TIE_QUERY[:5], WIDE_TIE_QUERY + "129", "Z00017Y"]
    return qs
