#!/usr/bin/env python3
"""Finds wide strings that collide under the interner's 64-bit hash (ngs_intern.hip, d_hash).

d_hash is FNV-1a over 32-bit characters, seeded by the length, with a bijective finaliser, so
two strings collide exactly when their states before the finaliser are equal. The state after the
last character c of a prefix state s is (s ^ c) * prime: two strings whose prefix states agree in
every bit above the 21 a code point can carry collide once their last characters differ by the xor
of the two prefix states. Across two lists (prefixes of 3 characters seeded for length 4, of 2
seeded for length 3) that is a 43-bit birthday: 2^24 samples each give a dozen pairs of lengths 4
and 3. Within one length FNV's multiply is weaker than that: prefixes whose first characters differ
by d and whose second differ by -870 d cancel above bit 21, so 2^24 samples hold millions of
same-length pairs and three-string classes among them; the search keeps the first few and one triple
(or records that it found none).

The length seeds the hash, so a pair of 3 characters stops colliding when a common suffix makes
both longer. For long colliding terms the search runs a second time under the seeds of lengths
3 + 8 and 4 + 8: the heads it finds (3 or 4 code points) have equal states, and collide with any
8 common characters behind them ("..._before_tail").

Writes tests/golden/collisions/intern_collisions.json: lists of code points only, every one a
scalar value >= 0x100 (no surrogates, nothing above 0x10FFFF), which the wide normalisation keeps as
it is. Every pair is confirmed with the plain-Python d_hash of tests/hash_cases.py before it is
written. Seeded: a rerun writes the same bytes. Under a minute on one core; the tests read the
file and never run the search.

    python tests/golden/make_golden_collisions.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import hash_cases as hc  # noqa: E402

SEED = 20240611
SAMPLES = 1 << 24
CJK_LO, CJK_HI = 0x4E00, 0x9FFF  # the prefixes' alphabet
FREE_BITS = 21                   # what the last character's xor can absorb
KEEP_SAME, KEEP_DIFF = 8, 4
TAIL = 8                         # the second search: heads that collide with 8 more characters behind them
PAD = [0x41] * TAIL
OUT = os.path.join(ROOT, "tests", "golden", "collisions", "intern_collisions.json")

PRIME = np.uint64(hc.FNV_PRIME)


def states(prefixes, length):
    """d_hash's state of a string of `length` characters after the prefix (one row each)."""
    h = np.full(len(prefixes), hc.FNV_OFFSET ^ (length * hc.GOLDEN64 & hc.M64), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for col in prefixes.T:
            h = (h ^ col) * PRIME
    return h


def scalar(c):
    return 0x100 <= c <= 0x10FFFF and not 0xD800 <= c <= 0xDFFF


def absorb(delta):
    """Last characters (a, b) with a ^ b == delta, both scalar values >= 0x100."""
    for hi in range(0, 16):
        for lo in range(CJK_LO, CJK_LO + 256):
            a = (hi << 16) | lo
            if scalar(a) and scalar(a ^ delta):
                return a, a ^ delta
    raise AssertionError(f"no last characters absorb {delta:#x}")


def finish(pa, sa, pb, sb, tail):
    a, b = absorb(int(sa) ^ int(sb))
    x, y = [int(c) for c in pa] + [a], [int(c) for c in pb] + [b]
    assert x != y and hc.d_hash(x + PAD[:tail]) == hc.d_hash(y + PAD[:tail]), (x, y)
    assert all(scalar(c) for c in x + y)
    return [x, y]


def dump(doc):
    """One key per line, lists of code points on one line each."""
    lines = []
    for k, v in doc.items():
        if isinstance(v, list) and v and isinstance(v[0], list):
            rows = ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in v)
            lines.append(f" {json.dumps(k)}: [\n{rows}\n ]")
        else:
            lines.append(f" {json.dumps(k)}: {json.dumps(v)}")
    return "{\n" + ",\n".join(lines) + "\n}\n"


def search(p2, p3, tail):
    """Collisions among strings of 3 + tail characters and between 4 + tail and 3 + tail: the heads
    (3 or 4 code points), equal in state after the head, so any common `tail` characters keep them."""
    s33 = states(p2, 3 + tail)  # after 2 characters
    s43 = states(p3, 4 + tail)  # after 3 characters

    # same length: neighbours of one class in the sorted order
    cls = s33 >> np.uint64(FREE_BITS)
    order = np.argsort(cls, kind="stable")
    sc = cls[order]
    eq = np.nonzero(sc[1:] == sc[:-1])[0]
    same, triple, used = [], None, set()
    for i in eq:
        if len(same) >= KEEP_SAME and triple is not None:
            break
        a, b = order[i], order[i + 1]
        if (p2[a] == p2[b]).all():
            continue  # one prefix drawn twice
        if i + 2 < len(sc) and sc[i + 2] == sc[i] and triple is None:
            c = order[i + 2]
            if not (p2[c] == p2[a]).all() and not (p2[c] == p2[b]).all():
                # the third last character follows from the first: it may fail to be a scalar value
                x, y = finish(p2[a], s33[a], p2[b], s33[b], tail)
                z = [int(v) for v in p2[c]] + [x[-1] ^ int(s33[a]) ^ int(s33[c])]
                if scalar(z[-1]) and hc.d_hash(z + PAD[:tail]) == hc.d_hash(x + PAD[:tail]):
                    triple = [x, y, z]
        pa, pb = tuple(map(int, p2[a])), tuple(map(int, p2[b]))
        if len(same) < KEEP_SAME and pa not in used and pb not in used:  # every string in one pair only
            used.update((pa, pb))
            same.append(finish(p2[a], s33[a], p2[b], s33[b], tail))
    assert len(same) >= 4, f"{len(same)} same-length pairs: raise SAMPLES"

    # lengths 4 and 3: both lists in one sort, neighbours from different lists
    both = np.concatenate([s43 >> np.uint64(FREE_BITS), cls])
    order = np.argsort(both, kind="stable")
    sb = both[order]
    long4 = order < SAMPLES
    eq = np.nonzero((sb[1:] == sb[:-1]) & (long4[1:] != long4[:-1]))[0]
    diff = []
    for i in eq:
        a, b = sorted((int(order[i]), int(order[i + 1])))
        diff.append(finish(p3[a], s43[a], p2[b - SAMPLES], s33[b - SAMPLES], tail))
    assert len(diff) >= 2, f"{len(diff)} pairs of different lengths: raise SAMPLES"
    return same[:KEEP_SAME], diff[:KEEP_DIFF], triple


def main():
    rng = np.random.default_rng(SEED)
    p2 = rng.integers(CJK_LO, CJK_HI + 1, size=(SAMPLES, 2), dtype=np.uint64)
    p3 = rng.integers(CJK_LO, CJK_HI + 1, size=(SAMPLES, 3), dtype=np.uint64)
    same, diff, triple = search(p2, p3, 0)
    same8, diff8, _ = search(p2, p3, TAIL)
    doc = {
        "source": "tests/golden/make_golden_collisions.py: birthday search on d_hash's state (ngs_intern.hip)",
        "seed": SEED,
        "samples": SAMPLES,
        "same_length": same,
        "different_length": diff,
        "triple": triple,
        "triple_note": None if triple else
        f"no three of the {SAMPLES} prefixes gave a triple of scalar values: the A, B, A runs of the tests are "
        "made from pairs",
        "tail": TAIL,
        "same_length_before_tail": same8,
        "different_length_before_tail": diff8,
    }
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(dump(doc))
    print(f"{OUT}: {len(same)} + {len(same8)} same-length pairs, {len(diff)} + {len(diff8)} of lengths 4 and 3, "
          f"triple: {bool(triple)}; {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
