"""Fabricated candidate blocks for the matching stage (ngsMatchDevice), shared by the host tests (the
header's routines under sanitizers, the model against itself) and the GPU tests (the kernels)."""
from __future__ import annotations

import random

import numpy as np

JUNK = 0xDEADBEEF
VALUES = (-1.0, -0.0, 0.0, 0.25, 0.5, 0.75, 1.0)  # few values: ties decide
RANDOM_STRIDES = (1, 3, 64, 65, 130)


def _case(name, n_a, n_b, first, rows, stride, counts=None):
    """rows: [[(b, value)]] -> (name, n_a, n_b, first, n, stride, counts, keys, values as fp32)."""
    n = len(rows)
    keys = np.full(n * stride, JUNK, dtype=np.uint32)
    values = np.full(n * stride, 7.0, dtype=np.float32)  # junk past a row's count: larger than any value
    cnt = np.zeros(n, dtype=np.uint32)
    for i, r in enumerate(rows):
        assert len(r) <= stride
        keys[i * stride:i * stride + len(r)] = [b for b, _ in r]
        values[i * stride:i * stride + len(r)] = [v for _, v in r]
        cnt[i] = len(r)
    if counts is not None:
        cnt = np.array(counts, dtype=np.uint32)
    return (name, n_a, n_b, first, n, stride, cnt, keys, values)


def random_case(stride: int):
    """300 source and 200 target ids; the block starts at key 5 and runs to id 314, past the sources.
    Row counts 0 .. stride + 2 (a count above the stride reads as the stride: every cell holds a record
    then), ids up to 219 (past the targets), one b twice in every seventh row."""
    rng = random.Random(0x3A7C + stride)
    n_a, n_b, first, n = 300, 200, 5, 310
    rows, counts = [], []
    for i in range(n):
        c = rng.randrange(0, stride + 3)
        row = [(rng.randrange(n_b + 20), rng.choice(VALUES)) for _ in range(stride if c > stride else c)]
        if i % 7 == 0 and len(row) >= 2:
            row[-1] = (row[0][0], rng.choice(VALUES))
        rows.append(row)
        counts.append(c)
    return _case(f"random-{stride}", n_a, n_b, first, rows, stride, counts)


def chain_case():
    """70 rows: row i offers b_i at 1 - 0.01 i and b_(i+1) at 1 - 0.01 i - 0.005. Row i holds the bid at
    b_(i+1) until it has taken b_i, so one row matches per round: 70 rounds and the empty one."""
    rows = [[(i + 1, np.float32(1.0 - 0.01 * i - 0.005)), (i, np.float32(1.0 - 0.01 * i))] for i in range(70)]
    return _case("chain", 70, 71, 0, rows, 2)


def contention_case():
    """1,000 rows whose first choice is b = 0 (one value: the smallest a has it) and whose second is a + 1."""
    rows = [[(0, 1.0), (a + 1, 0.5)] for a in range(1000)]
    return _case("contention", 1000, 1001, 0, rows, 3)


def cases():
    return [random_case(s) for s in RANDOM_STRIDES] + [chain_case(), contention_case()]


def cuts_of(n: int, seed: int, parts: int = 5):
    """Random row boundaries 0 = c_0 <= ... <= c_k = n (an empty block among them)."""
    rng = random.Random(seed)
    c = sorted([0, n] + [rng.randrange(n + 1) for _ in range(parts - 1)])
    c.insert(2, c[1])  # an empty block
    return c
