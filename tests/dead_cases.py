"""The planted blocks of the dead-key tests (tests/test_set_dead_host.py, tests/test_gpu_set_dead.py):
the smallest shapes at which the in-place compaction of k_drop_dead can go wrong. A case is (name,
block, limits); the block is dead_ref's dict."""
from __future__ import annotations

import random

import numpy as np

import dead_ref

ONE_WAVE = 256   # kSetOneWaveRecords: a launch whose rows hold more runs a workgroup of THREADS
THREADS = 256    # kSetThreads
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 600, 1100)
N_KEYS = 4090    # not a multiple of 32: the last mask word has bits past the keys


def _pools(rng):
    """A quarter of the keys dead at random, with the mask word edges planted: 31 and 64 dead, 32 and 63
    live; the bits of the last word past N_KEYS are set and mean nothing."""
    dead = (set(rng.sample(range(N_KEYS), N_KEYS // 4)) | {0, 31, 64}) - {30, 32, 33, 62, 63, 65}
    words = dead_ref.mask(N_KEYS, sorted(dead) + list(range(N_KEYS, 32 * ((N_KEYS + 31) // 32))))
    live = [k for k in range(N_KEYS) if k not in dead]
    return sorted(dead), live, words


def _row(pattern, dead, live, rng):
    """Key ids for a row of booleans (True: a dead key), distinct within the row where the pools allow."""
    d, l = rng.sample(dead, min(len(dead), sum(pattern))), rng.sample(live, min(len(live), len(pattern) - sum(pattern)))
    di = li = 0
    out = []
    for x in pattern:
        if x:
            out.append(d[di % len(d)])
            di += 1
        else:
            out.append(l[li % len(l)])
            li += 1
    return out


def _block(rows, stride, words, n_keys, counts=None, seed=1):
    """rows: lists of key ids (a row longer than the stride is cut: its count stays above the stride).
    The cells past a row's records hold ids of dead and live keys that must never be looked at."""
    rng = random.Random(seed)
    n = len(rows)
    keys = np.array([rng.randrange(0, max(1, n_keys)) for _ in range(n * stride)], dtype=np.uint32)
    for i, r in enumerate(rows):
        r = r[:stride]
        keys[i * stride:i * stride + len(r)] = r
    # every record's score is its own: a moved record is recognised by it
    scores = (np.uint32(0x3F000000) + np.arange(n * stride, dtype=np.uint32) * np.uint32(7)).astype(np.uint32)
    counts = [len(r) for r in rows] if counts is None else counts
    return {"n": n, "stride": stride, "counts": np.array(counts, dtype=np.uint32), "keys": keys, "scores": scores,
            "n_keys": n_keys, "dead": words}


def patterns(c, chunk):
    """The dead / live patterns of a row of c records compacted in chunks of `chunk`."""
    run = [False] * c
    for r in range(max(0, chunk - 6), min(c, chunk + 5)):  # a dead run across the first chunk boundary
        run[r] = True
    return {"all": [True] * c, "none": [False] * c, "first": [r == 0 for r in range(c)],
            "last": [r == c - 1 for r in range(c)], "alternate": [r % 2 == 0 for r in range(c)], "run": run}


def cases():
    rng = random.Random(0xDEAD)
    dead, live, words = _pools(rng)
    out = []
    # every count under every pattern, on each side of the one-wave cut-over: stride 256 runs one wave
    # (a count above the stride is read as the stride), stride 1,150 a workgroup carrying its base over
    # up to five chunks
    for name, stride, chunk in (("wave", ONE_WAVE, 64), ("group", 1150, THREADS)):
        for pat in ("all", "none", "first", "last", "alternate", "run"):
            rows, counts = [], []
            for c in COUNTS:
                rows.append(_row(patterns(min(c, stride), chunk)[pat], dead, live, rng))
                counts.append(c)
            b = _block(rows, stride, words, N_KEYS, counts, seed=len(out))
            mid = sum(1 for k in rows[5] if k in live)  # the live records of the row of 255
            out.append((f"{name}-{pat}", b, (0, 1, 10, mid, max(1, mid - 1), 300)))
    # random rows, a quarter dead: the general case, one wave and a workgroup
    for name, stride in (("wave-random", 200), ("group-random", 700)):
        rows = [[rng.randrange(N_KEYS) for _ in range(rng.choice((stride, stride, stride - 1, stride // 2, 65)))]
                for _ in range(8)]
        counts = [len(r) if i % 3 else len(r) + 40 * (len(r) == stride) for i, r in enumerate(rows)]
        out.append((name, _block(rows, stride, words, N_KEYS, counts, seed=len(out)), (0, 1, 100, 164, stride)))
    # the mask word edges, ids at and past n_keys (kept, nothing read: the set bits past N_KEYS in the
    # last word included), a count above the stride
    edge = [30, 31, 32, 33, 62, 63, 64, 65, 0, N_KEYS - 1, N_KEYS, N_KEYS + 3, 4095, 4096, 0x7FFFFFFF, 0xFFFFFFFF]
    out.append(("edges", _block([edge, edge[::-1], edge[:9], []], 16, words, N_KEYS, [16, 99, 9, 0], seed=77),
                (0, 1, 5, 16)))
    # no keys and no mask: every record is kept
    out.append(("no-mask", _block([[5, 6, 7], [1] * 70, []], 70, None, 0, seed=78), (0, 2, 70)))
    # stride 0 and a block of one cell
    out.append(("stride-0", _block([[], []], 0, words, N_KEYS, [0, 5], seed=79), (0, 3)))
    out.append(("stride-1", _block([[0], [32], []], 1, words, N_KEYS, [1, 7, 0], seed=80), (0, 1, 2)))
    return out


def random_small(rng):
    """(block, limit): a few short rows over a small mask."""
    n_keys = rng.choice((0, 1, 31, 32, 33, 100))
    dead = [k for k in range(n_keys) if rng.random() < rng.choice((0.0, 0.3, 0.9, 1.0))]
    words = dead_ref.mask(n_keys, dead) if n_keys else None
    stride = rng.randrange(0, 12)
    n = rng.randrange(0, 4)
    rows = [[rng.randrange(0, n_keys + 3) for _ in range(rng.randrange(0, stride + 1))] for _ in range(n)]
    counts = [len(r) + rng.choice((0, 0, 5)) * (len(r) == stride) for r in rows]
    return _block(rows, stride, words, n_keys, counts, seed=rng.randrange(1 << 30)), rng.choice((0, 0, 1, 2, 5, 11, 12))
