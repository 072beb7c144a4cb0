"""Reference of the edit-distance similarity (include/ngram_search.h, "Edit-distance similarity"),
in Python and numpy alone, for tests/test_sim_host.py and tests/test_gpu_sim.py.

Strings are sequences of ints: bytes of a narrow index, UTF-32 units of a wide one. The value is
    sim(Q, T) = float32(1) - float32(d) / float32(max(m, L))
with d the unit-cost Levenshtein distance from a two-row DP (`lev`; `lev_batch` runs the same two
rows over many pairs at once), and a record's similarity the largest over its key's terms.
"""
from __future__ import annotations

import numpy as np

# the validChar set every index is built with (stringsearchlib_amd/csrc/ngs_index.cpp:18)
DEFAULT_VALID = b".%$ @0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
SIM_MAX_QUERY = 4096
RERANK_MAX_STRIDE = 4096
SIM_WILDCARD = np.float32(1.0)
SIM_NONE = np.float32(-1.0)


def units(s, wide: bool = False) -> list[int]:
    """bytes / str / a sequence of ints -> the characters as ints."""
    if isinstance(s, (bytes, bytearray)):
        return list(s)
    if isinstance(s, str):
        return [ord(c) for c in s] if wide else list(s.encode("latin-1"))
    return [int(c) & 0xFFFFFFFF for c in s]


def _space(c: int) -> bool:
    return c == 32 or 9 <= c <= 13


def _esc(c: int, valid, wide: bool) -> int:
    if not wide or c < 128:
        return c if c in valid else 32
    return 32 if c > 0x10FFFF else c


def _upper(c: int) -> int:
    return c - 32 if 97 <= c <= 122 else c


def is_wildcard(raw) -> bool:
    return len(raw) == 0 or (len(raw) == 1 and raw[0] == ord("*"))


def normalise(raw, valid=DEFAULT_VALID, wide: bool = False) -> tuple:
    """escapeBlank with `valid`, trim, toupper: Q of a query, T of an indexed word."""
    vs = frozenset(valid)
    e = [_esc(c, vs, wide) for c in raw]
    a, b = 0, len(e)
    while a < b and _space(e[a]):
        a += 1
    while b > a and _space(e[b - 1]):
        b -= 1
    return tuple(_upper(c) for c in e[a:b])


def lev(a, b) -> int:
    """Unit-cost Levenshtein distance, two rows."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, cb in enumerate(b, 1):
            cur[j] = min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def _lev_block(qs, ts) -> np.ndarray:
    n = len(qs)
    m = np.array([len(q) for q in qs], dtype=np.int64)
    ln = np.array([len(t) for t in ts], dtype=np.int64)
    mm, w = int(m.max()), int(ln.max())
    q = np.full((n, max(mm, 1)), -1, dtype=np.int64)
    t = np.full((n, w), -2, dtype=np.int64)
    for i in range(n):
        q[i, :len(qs[i])] = qs[i]
        t[i, :len(ts[i])] = ts[i]
    idx = np.arange(w + 1, dtype=np.int64)
    prev = np.tile(idx, (n, 1))
    for i in range(1, mm + 1):
        x = np.minimum(prev[:, :-1] + (t != q[:, i - 1:i]), prev[:, 1:] + 1)
        # cur[j] = min(x[j], cur[j - 1] + 1): a running minimum of the values less their column
        y = np.concatenate((np.full((n, 1), i, dtype=np.int64), x), axis=1) - idx
        cur = np.minimum.accumulate(y, axis=1) + idx
        prev = np.where((i <= m)[:, None], cur, prev)
    return prev[np.arange(n), ln]


def lev_batch(qs, ts, block: int = 2048) -> np.ndarray:
    """lev() of every pair (qs[i], ts[i]): the same two rows, over a block of pairs at once."""
    n = len(qs)
    out = np.zeros(n, dtype=np.int64)
    groups: dict = {}  # pairs of like sizes together: a block is padded to its longest strings
    for i in range(n):
        groups.setdefault((len(qs[i]).bit_length(), len(ts[i]).bit_length()), []).append(i)
    for idx in groups.values():
        for a in range(0, len(idx), block):
            sel = idx[a:a + block]
            out[sel] = _lev_block([qs[i] for i in sel], [ts[i] for i in sel])
    return out


def sim_value(d, m, ln) -> np.float32:
    if max(m, ln) == 0:  # (no indexed term is empty; two empty strings are equal)
        return np.float32(1.0)
    return np.float32(1.0) - np.float32(d) / np.float32(max(m, ln))


def key_terms(words, row_size: int = 1, weights=None, wide: bool = False) -> dict:
    """The index's keys and their terms from what was indexed: {trimmed master key (tuple of ints):
    set of normalised terms}. A pair exists for every word of a row with a non-zero weight (an
    alias that normalises to nothing has none); a key without a pair is not in the index."""
    out: dict = {}
    for i in range(0, len(words), row_size):
        if words[i] is None:
            continue
        raw = units(words[i], wide)
        a, b = 0, len(raw)
        while a < b and raw[a] < 128 and _space(raw[a]):
            a += 1
        while b > a and raw[b - 1] < 128 and _space(raw[b - 1]):
            b -= 1
        if a == b:
            continue
        key = tuple(raw[a:b])
        for j in range(i, min(i + row_size, len(words))):
            if words[j] is None:
                continue
            t = normalise(raw[a:b] if j == i else units(words[j], wide), DEFAULT_VALID, wide)
            if j != i and not t:
                continue
            if weights is not None and weights[j] == 0.0:
                continue
            out.setdefault(key, set()).add(t)
    return out


def record_sims(pairs, valid=DEFAULT_VALID, wide: bool = False) -> np.ndarray:
    """pairs: [(raw query, terms of the key or None for a key id outside the index)] -> float32 sims.
    Terms are the normalised terms of the key (key_terms); an empty term is not compared."""
    out = np.full(len(pairs), SIM_NONE, dtype=np.float32)
    qn: dict = {}
    jobs, where = [], []
    for r, (raw, terms) in enumerate(pairs):
        raw = tuple(raw)
        if is_wildcard(raw):  # every record, whatever its key id
            out[r] = SIM_WILDCARD
            continue
        if terms is None:
            continue
        if raw not in qn:
            qn[raw] = normalise(raw, valid, wide)
        q = qn[raw]
        if len(q) > SIM_MAX_QUERY:
            continue
        for t in terms:
            if len(t):
                jobs.append((q, t))
                where.append(r)
    uniq = sorted(set(jobs), key=lambda p: (len(p[0]), len(p[1])))
    d = lev_batch([p[0] for p in uniq], [p[1] for p in uniq]) if uniq else []
    dist = {p: int(x) for p, x in zip(uniq, d)}
    for (q, t), r in zip(jobs, where):
        s = sim_value(dist[(q, t)], len(q), len(t))
        if s > out[r]:
            out[r] = s
    return out


def rerank(keys, scores, sims, min_sim):
    """One query's records after ngsRerankDevice: sim < min_sim dropped, the rest by (sim desc,
    position asc). Returns (keys, scores, sims) lists."""
    ms = np.float32(min_sim)
    kept = [i for i in range(len(keys)) if not (np.float32(sims[i]) < ms)]
    kept.sort(key=lambda i: (-float(sims[i]), i))
    return [keys[i] for i in kept], [scores[i] for i in kept], [sims[i] for i in kept]
