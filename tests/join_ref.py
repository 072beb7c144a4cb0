"""Plain Python model of the self-join and its clusters (include/ngram_search.h, "Self-join on the
device"): what the tests of the join compare the library with.

* the expected row of key k is the oracle's full answer for k's string (limit 0) without k's own
  entry, cut to the limit;
* a sequential union-find gives every key the smallest id of its component.
"""
from __future__ import annotations

import numpy as np


# ---- the gather's layout ----
def query_offsets(lengths, cs: int = 1):
    """Byte offsets [0 .. n] of strings of those lengths (in characters of cs bytes), back to back."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + n * cs)
    return off


def offsets_from_key_off(key_off, first: int, n: int, cs: int = 1):
    """The formula the kernel uses: key_off counts one NUL per key."""
    return [(key_off[first + i] - key_off[first] - i) * cs for i in range(n + 1)]


# ---- drop-self ----
def drop_self(keys, scores, count: int, stride: int, self_id: int, limit: int):
    """One row: (new count, keys, scores) with the first record of key self_id removed and the row cut
    to `limit` (0: no cut); a count above the stride is read as the stride."""
    count = min(count, stride)
    k, s = list(keys[:count]), list(scores[:count])
    if self_id in k:
        p = k.index(self_id)
        del k[p], s[p]
    if limit:
        k, s = k[:limit], s[:limit]
    return len(k), k, s


# ---- clusters ----
def block_edges(counts, keys, n: int, stride: int, first: int):
    return [(first + i, int(keys[i * stride + r])) for i in range(n) for r in range(min(int(counts[i]), stride))]


def labels(n_labels: int, edges):
    """labels[k] = smallest id of k's component; edges with an end >= n_labels are ignored."""
    parent = list(range(n_labels))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges:
        if a >= n_labels or b >= n_labels:
            continue
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return [find(k) for k in range(n_labels)]


# ---- the oracle's full answers, a chunk of queries at a time on several threads ----
def oracle_full(oi, queries, thr: float, threads: int = 8, chunk: int = 256):
    """[(oracle key ids, fp32 scores)] per query at limit 0. oi: OracleIndex (bytes queries) or
    OracleIndexG (str / int-sequence queries)."""
    batch = oi.score_batch_raw if hasattr(oi, "score_batch_raw") else oi.score_batch
    out = []
    for a in range(0, len(queries), chunk):
        qs = queries[a:a + chunk]
        counts, keys, scores, cap = batch(qs, thr, 0, threads)
        k = np.frombuffer(keys, dtype=np.uint32)
        s = np.frombuffer(scores, dtype=np.float32)
        for i in range(len(qs)):
            c = counts[i]
            out.append((k[i * cap:i * cap + c].copy(), s[i * cap:i * cap + c].copy()))
    return out


def join_row_np(ids, bits, self_id: int, limit: int):
    """(key ids, fp32 bits) of a whole ranking -> the row the join answers for key self_id."""
    at = np.flatnonzero(ids == self_id)
    if at.size:
        ids, bits = np.delete(ids, at[0]), np.delete(bits, at[0])
    return (ids[:limit], bits[:limit]) if limit else (ids, bits)


def oracle_join(oi, key_strings, id_of_oracle_key, first: int, count: int, thr: float, limits, threads: int = 8):
    """{limit: rows}, rows[i] = (key ids, fp32 score bits) as uint32 arrays, of key first + i: the
    oracle's full answer for key_strings[first + i] (limit 0) with the oracle's ids mapped through
    id_of_oracle_key (a uint32 array), the key's own entry removed, cut to the limit."""
    full = oracle_full(oi, key_strings[first:first + count], thr, threads)
    rows = {lim: [] for lim in limits}
    for i, (k, s) in enumerate(full):
        ids = id_of_oracle_key[k].astype(np.uint32) if len(k) else k
        for lim in limits:
            rows[lim].append(join_row_np(ids, s.view(np.uint32), first + i, lim))
    return rows


def rows_edges(rows, first: int = 0):
    return [(first + i, int(b)) for i, (ids, _) in enumerate(rows) for b in ids]
