"""Reference of the similarity's metrics and of the matched term (include/ngram_search.h, "The
similarity by a metric"), in Python and numpy alone, for tests/test_metric_host.py and
tests/test_gpu_metric.py. Strings are sequences of ints, as in sim_ref.

    levenshtein  d = unit-cost Levenshtein,                        sim = 1 - d / max(m, L)
    osa          ... plus the swap of two adjacent characters at cost 1, no substring edited twice:
                 D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + [Q_i != T_j],
                               D[i-2][j-2] + 1 if Q_i = T_{j-1} and Q_{i-1} = T_j),  same sim
    partial      d = min over 0 <= a <= b <= L of Levenshtein(Q, T[a..b)),  sim = 1 - d / m (0 for m = 0)

`osa` and `partial` are the DPs cell by cell, straight from the definitions. `dist_batch` runs the
same DPs a row at a time over many pairs at once (numpy), which is what makes 4,096-character pairs
affordable; tests/test_metric_host.py holds the two forms against each other.
"""
from __future__ import annotations

import numpy as np

import sim_ref
from sim_ref import DEFAULT_VALID, SIM_MAX_QUERY, SIM_NONE, SIM_WILDCARD, key_terms, normalise, units  # noqa: F401

LEVENSHTEIN, OSA, PARTIAL = 0, 1, 2
METRICS = {"levenshtein": LEVENSHTEIN, "osa": OSA, "partial": PARTIAL}
NO_TERM = 0xFFFFFFFF


def osa(a, b) -> int:
    """Optimal string alignment distance: the full table."""
    m, n = len(a), len(b)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        D[i][0] = i
    for j in range(n + 1):
        D[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                D[i][j] = min(D[i][j], D[i - 2][j - 2] + 1)
    return D[m][n]


def partial(q, t) -> int:
    """min over substrings T[a..b) of Levenshtein(Q, T[a..b)): a free start is a zero top row, a free
    end the least of the last row (column 0, the empty substring, included)."""
    m, n = len(q), len(t)
    prev = [0] * (n + 1)
    for i in range(1, m + 1):
        cur = [i] + [0] * n
        for j in range(1, n + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (q[i - 1] != t[j - 1]))
        prev = cur
    return min(prev)


def partial_by_definition(q, t) -> int:
    """The definition itself, every substring: for tiny strings only."""
    return min(sim_ref.lev(q, t[a:b]) for a in range(len(t) + 1) for b in range(a, len(t) + 1))


def dist(q, t, metric: int) -> int:
    return (sim_ref.lev, osa, partial)[metric](q, t)


def _block(qs, ts, metric: int) -> np.ndarray:
    n = len(qs)
    m = np.array([len(q) for q in qs], dtype=np.int64)
    ln = np.array([len(t) for t in ts], dtype=np.int64)
    mm, mmin, w = int(m.max()), int(m.min()), int(ln.max())
    q = np.full((n, max(mm, 1)), -1, dtype=np.int64)
    t = np.full((n, max(w, 1)), -2, dtype=np.int64)[:, :w]
    for i in range(n):
        q[i, :len(qs[i])] = qs[i]
        t[i, :len(ts[i])] = ts[i]
    idx = np.arange(w + 1, dtype=np.int64)
    prev = np.zeros((n, w + 1), dtype=np.int64) if metric == PARTIAL else np.tile(idx, (n, 1))
    prev2 = prev
    for i in range(1, mm + 1):
        qi = q[:, i - 1:i]
        x = np.minimum(prev[:, :-1] + (t != qi), prev[:, 1:] + 1)  # columns 1 .. w: from the row above
        if metric == OSA and i >= 2 and w >= 2:
            # column j >= 2: Q_i = T_{j-1} and Q_{i-1} = T_j
            swap = (t[:, :-1] == qi) & (t[:, 1:] == q[:, i - 2:i - 1])
            x[:, 1:] = np.where(swap, np.minimum(x[:, 1:], prev2[:, :-2] + 1), x[:, 1:])
        # cur[j] = min(x[j], cur[j - 1] + 1): a running minimum of the values less their column
        y = np.concatenate((np.full((n, 1), i, dtype=np.int64), x), axis=1) - idx
        cur = np.minimum.accumulate(y, axis=1) + idx
        if i <= mmin:
            prev2, prev = prev, cur
        else:  # the shorter queries of the block are done: their rows stay
            live = (i <= m)[:, None]
            prev2 = np.where(live, prev, prev2)
            prev = np.where(live, cur, prev)
    if metric == PARTIAL:
        return np.where(idx[None, :] <= ln[:, None], prev, np.iinfo(np.int64).max).min(axis=1)
    return prev[np.arange(n), ln]


def dist_batch(qs, ts, metric: int, block: int = 2048) -> np.ndarray:
    """dist() of every pair (qs[i], ts[i]): the same rows, over a block of pairs of like sizes at once."""
    n = len(qs)
    out = np.zeros(n, dtype=np.int64)
    groups: dict = {}
    for i in range(n):
        groups.setdefault((len(qs[i]).bit_length(), len(ts[i]).bit_length()), []).append(i)
    for idx in groups.values():
        for a in range(0, len(idx), block):
            sel = idx[a:a + block]
            out[sel] = _block([qs[i] for i in sel], [ts[i] for i in sel], metric)
    return out


def sim_value(d, m, ln, metric: int) -> np.float32:
    if metric == PARTIAL:
        return np.float32(0.0) if m == 0 else np.float32(1.0) - np.float32(d) / np.float32(m)
    return sim_ref.sim_value(d, m, ln)


def record_sims(pairs, metric: int, term_ids=None, valid=DEFAULT_VALID, wide: bool = False):
    """pairs: [(raw query, terms of the key or None for a key id outside the index)] -> (float32 sims,
    matched terms). The matched term of a record is the term (tuple of ints) that attains its similarity,
    among several of one fp32 value the one with the smallest term_ids[term]; None where no term was
    compared. Without term_ids the second value is None."""
    out = np.full(len(pairs), SIM_NONE, dtype=np.float32)
    best = [None] * len(pairs)
    qn: dict = {}
    jobs, where = [], []
    for r, (raw, terms) in enumerate(pairs):
        raw = tuple(raw)
        if sim_ref.is_wildcard(raw):
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
    d = dist_batch([p[0] for p in uniq], [p[1] for p in uniq], metric) if uniq else []
    dmap = {p: int(x) for p, x in zip(uniq, d)}
    for (q, t), r in zip(jobs, where):
        s = sim_value(dmap[(q, t)], len(q), len(t), metric)
        if best[r] is None or s > out[r] or (s == out[r] and term_ids is not None and term_ids[t] < term_ids[best[r]]):
            out[r] = s
            best[r] = t
    return out, (best if term_ids is not None else None)


def rerank(keys, scores, sims, terms, min_sim):
    """One query's records after ngsRerankDeviceM: sim < min_sim dropped, the rest by (sim desc, position
    asc), the terms moving with their records. Returns (keys, scores, sims, terms) lists."""
    ms = np.float32(min_sim)
    kept = [i for i in range(len(keys)) if not (np.float32(sims[i]) < ms)]
    kept.sort(key=lambda i: (-float(sims[i]), i))
    return ([keys[i] for i in kept], [scores[i] for i in kept], [sims[i] for i in kept], [terms[i] for i in kept])
