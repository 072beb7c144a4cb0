"""Fabricated result blocks for the merge of index sets (ngsMergeResultsDevice), shared by the host tests
(the model against a brute-force sort, ngs_set.h's routine under sanitizers) and the GPU tests (the
kernel). Every row of every part is in merge order, as ngsSearchDevice writes it; the cells past a
row's count hold junk that sorts before everything, so a read past the count shows.

A case is (name, parts, n, limits); a part is set_ref's dict."""
from __future__ import annotations

import os
import random
import re
import struct

import numpy as np

import set_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "stringsearchlib_amd", "csrc", "ngs_set.h")
JUNK_KEY = 0xDEADBEEF
JUNK_SCORE = 0x7F7FFFFF  # FLT_MAX: ahead of every planted score but +inf and the NaN


def bits(*values):
    return [struct.unpack("<I", struct.pack("<f", v))[0] for v in values]


def constant(name: str) -> int:
    """A `constexpr uint32_t` of ngs_set.h: the kernel's own cut-over constants."""
    m = re.search(rf"constexpr\s+uint32_t\s+{name}\s*=\s*(\d+)u?;", open(HEADER).read())
    assert m, name
    return int(m.group(1))


ONE_WAVE = constant("kSetOneWaveRecords")
LDS = constant("kSetLdsRecords")
MAX_PARTS = constant("kSetMaxParts")
PLAIN = bits(100.0, 87.5, 50.0, 33.25, 12.5)  # few scores: ties decide
# +0, a subnormal, 100, the float above 100, +inf, -0, a negative value, a quiet NaN
ODD = bits(0.0) + [0x00000001] + bits(100.0) + [bits(100.0)[0] + 1] + bits(float("inf"), -0.0, -3.5) + [0x7FC00000]


def part(rng, n, stride, n_keys, base, counts, scores, lens=None, id_span=None):
    """One part: row i holds min(counts[i], stride) records of distinct ids below id_span (default
    n_keys) with scores drawn from `scores`, in merge order. lens: the length table (default: ascending
    with the id, as key ids are ranks by length, in runs so that lengths tie)."""
    if lens is None:
        lens = [3 + k // 4 for k in range(n_keys)]
    lens = np.array(lens, dtype=np.uint32)
    keys = np.full(n * stride, JUNK_KEY, dtype=np.uint32)
    sc = np.full(n * stride, JUNK_SCORE, dtype=np.uint32)
    span = id_span or n_keys
    for i in range(n):
        c = min(int(counts[i]), stride)
        recs = [(k, rng.choice(scores)) for k in rng.sample(range(span), c)]
        img = lambda b: int(set_ref.order_bits(np.uint32(b)))
        recs.sort(key=lambda r: (-img(r[1]), int(lens[r[0]]) if r[0] < n_keys else set_ref.NO_LEN, r[0]))
        keys[i * stride:i * stride + c] = [k for k, _ in recs]
        sc[i * stride:i * stride + c] = [b for _, b in recs]
    return dict(counts=np.array(counts, dtype=np.uint32), keys=keys, scores=sc, stride=stride, base=base, lens=lens)


def cases():
    rng = random.Random(0x5E7)
    out = []
    # P = 1 with a base: the identity plus the base; a count above the stride; the limit cuts
    out.append(("one-part", [part(rng, 6, 7, 40, 1000, [7, 9, 0, 3, 100, 1], PLAIN)], 6, [0, 1, 3, 7, 100]))
    # P = 2, one score: the lengths decide
    out.append(("lengths", [part(rng, 4, 10, 30, 0, [10, 4, 0, 7], PLAIN[:1]),
                            part(rng, 4, 10, 30, 30, [10, 9, 3, 0], PLAIN[:1])], 4, [0, 1, 5, 20]))
    # P = 2, one score and one length: the part, then the id
    out.append(("part-then-id", [part(rng, 4, 10, 30, 0, [10, 4, 0, 7], PLAIN[:1], lens=[5] * 30),
                                 part(rng, 4, 10, 30, 30, [10, 9, 3, 0], PLAIN[:1], lens=[5] * 30)], 4,
                [0, 1, 5, 20]))
    # P = 3, strides 1, 7, 100: the middle part empty in every row, rows 2 and 5 empty in every part
    c0 = [1, 3, 0, 0, 1, 0, 1, 1]
    c2 = [100, 37, 0, 1, 120, 0, 64, 99]
    out.append(("uneven", [part(rng, 8, 1, 9, 0, c0, PLAIN), part(rng, 8, 7, 50, 9, [0] * 8, PLAIN),
                           part(rng, 8, 100, 300, 59, c2, PLAIN)], 8, [0, 1, 50, 101, 108]))
    # P = 16, stride 5, full rows: limits on a wave edge and at the total
    out.append(("sixteen", [part(rng, 8, 5, 20, 20 * p, [5] * 8, PLAIN) for p in range(MAX_PARTS)], 8,
                [1, 63, 64, 65, 80, 81]))
    # P = 4, stride 3,000, full rows: everything out, a limit above the stride, the one-wave cut-over
    big = [part(rng, 3, 3000, 3500, 3500 * p, [3000, 3001, 3000], PLAIN) for p in range(4)]
    w = ONE_WAVE // 4
    out.append(("large", big, 3, [0, 4096, 1, w - 1, w, w + 1]))
    # ... and rows that hold the LDS cut-over's records, one fewer and one more (at limit 0 and above the stride)
    full = (LDS - 2) // 3000  # parts with full rows below the cut-over
    edge = LDS - 3000 * full
    assert 1 <= full <= 2 and 1 < edge < 3000
    rows = [[3000] * 4 if p < full else [edge - 1, edge, edge + 1, 3000] if p == full else [0, 0, 0, 3000]
            for p in range(4)]
    out.append(("lds-edge", [part(rng, 4, 3000, 3500, 3500 * p, rows[p], PLAIN) for p in range(4)], 4, [0, 4096]))
    # ids past the length table: their length reads as 0xFFFFFFFF and the output id is base + k
    out.append(("ids-past", [part(rng, 5, 12, 10, 7, [12, 5, 0, 12, 9], PLAIN[:2], id_span=25),
                             part(rng, 5, 12, 0, 0xFFFFFFF0, [3, 0, 12, 12, 1], PLAIN[:2], lens=[], id_span=40)], 5,
                [0, 1, 6, 24]))
    # the odd score bits
    out.append(("score-bits", [part(rng, 6, 16, 40, 40 * p, [16, 8, 0, 16, 3, 11], ODD) for p in range(3)], 6,
                [0, 1, 7, 48]))
    # a limit inside a tie class that spans all parts
    out.append(("tie-span", [part(rng, 4, 6, 12, 12 * p, [6, 6, 2, 5], PLAIN[:1], lens=[4] * 12) for p in range(4)],
                4, [1, 3, 10, 13, 0]))
    return out


def random_small(rng):
    """A small random case for the model check: (parts, n, limit)."""
    n = rng.randrange(1, 4)
    parts = []
    for p in range(rng.randrange(1, 5)):
        stride = rng.randrange(0, 7)
        n_keys = rng.randrange(0, 9)
        span = max(n_keys + rng.randrange(0, 4), stride)  # ids past the table among them
        counts = [rng.randrange(0, stride + 3) for _ in range(n)]
        lens = sorted(rng.randrange(1, 4) for _ in range(n_keys))
        parts.append(part(rng, n, stride, n_keys, rng.randrange(0, 50), counts, rng.choice((PLAIN[:2], ODD)),
                          lens=lens, id_span=span))
    return parts, n, rng.choice((0, 1, 2, 5, 30))
