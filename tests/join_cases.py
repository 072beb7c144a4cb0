"""Fabricated result blocks for the drop-self and cluster stages of the self-join, shared by the host
tests (the header's routines under sanitizers) and the GPU tests (the kernels)."""
from __future__ import annotations

import random

import numpy as np

DROP_STRIDES = (1, 63, 64, 65, 129, 4097)
DROP_FIRST = 777  # a non-zero firstKey
JUNK = 0xDEADBEEF


def drop_limits(stride: int):
    return sorted({0, 1, stride - 1, stride})


def drop_block(stride: int):
    """(counts[n], keys[n * stride], scores[n * stride]) as numpy arrays: one row per (count, place of
    the row's own record). Counts: 0, 1, about half, the stride, above the stride. Places: the first
    cell, cells 63, 64 and 65, the last cell, absent. The cells past a row's count hold junk, the
    row's own id among it: nothing there may be read as a record. Row i's own id is DROP_FIRST + i;
    the other ids are distinct and the scores follow their keys (score = id / 8)."""
    shapes = []
    for count in sorted({0, 1, stride // 2 + 1, stride, stride + 5}):
        live = min(count, stride)
        for place in sorted({p for p in (0, 63, 64, 65, live - 1) if 0 <= p < live}) + [None]:
            shapes.append((count, place))
    n = len(shapes)
    counts = np.array([c for c, _ in shapes], dtype=np.uint32)
    keys = np.zeros(n * stride, dtype=np.uint32)
    for i, (count, place) in enumerate(shapes):
        row = 1_000_000 + i * 8192 + np.arange(stride, dtype=np.uint32)
        live = min(count, stride)
        row[live:] = DROP_FIRST + i  # junk past the count
        if place is not None:
            row[place] = DROP_FIRST + i
        keys[i * stride:(i + 1) * stride] = row
    scores = (keys.astype(np.float64) / 8.0).astype(np.float32)
    return counts, keys, scores


def cluster_cases():
    """[(name, n_labels, first, n, stride, counts, keys)]: row i holds edges first + i -> keys[i * stride + r]."""
    rng = random.Random(0xC1)
    cases = []

    def add(name, n_labels, first, rows, stride, counts=None):
        n = len(rows)
        keys = np.full(n * stride, JUNK, dtype=np.uint32)
        cnt = np.zeros(n, dtype=np.uint32)
        for i, r in enumerate(rows):
            keys[i * stride:i * stride + len(r)] = r
            cnt[i] = len(r)
        if counts is not None:
            cnt = np.array(counts, dtype=np.uint32)
        cases.append((name, n_labels, first, n, stride, cnt, keys))

    N = 5000
    add("chain", N, 0, [[i + 1] for i in range(N - 1)], 1)
    add("chain-reversed", N, 0, [[]] + [[i - 1] for i in range(1, N)], 1)
    add("star-onto-last", N, 0, [[N - 1] for _ in range(N - 1)], 1)
    add("star-onto-0", N, 0, [[0] for _ in range(N)], 1)
    half = N // 2
    add("two-chains-late-edge", N, 0,
        [[i + 1] if i not in (half - 1, N - 1) else ([] if i == half - 1 else [0]) for i in range(N)], 2)
    rows = []
    for i in range(600):
        p = rng.randrange(600) if i % 3 == 0 else i
        rows.append([i, p, p, i])
    add("self-and-repeated-edges", 600, 0, rows, 4)
    # ids >= n_labels on either end: rows 100.. (their own id is out) and keys past the labels
    rows = [[(i + 1) % 150, 100 + i, 0xFFFFFFFF] if i % 5 else [i // 5] for i in range(150)]
    add("ids-past-the-labels", 100, 0, rows, 3)
    # counts above the stride are read as the stride (every cell of the row holds a record)
    rows = [[rng.randrange(300), rng.randrange(300)] for _ in range(300)]
    add("counts-above-stride", 300, 0, rows, 2, counts=[2 + (i % 3) * 40 for i in range(300)])
    # a block of a larger library: rows 1000 .. 1499 of 2,000 labels, random partners, wide rows
    rows = [[rng.randrange(2000) for _ in range(rng.randrange(0, 4))] for _ in range(500)]
    add("offset-block", 2000, 1000, rows, 70)
    add("one-label", 1, 0, [[0], [0]], 1)
    return cases
