"""Plain Python model of linking two indexes (include/ngram_search.h, "Linking two indexes"): what the
tests of ngsMatchDevice and linkKeys compare the library with.

* an edge is (a, b, value); edges are ordered by value descending (by the order image of the fp32
  bits), then a ascending, then b ascending;
* `greedy` goes through the sorted edges and takes one iff both its ends are free; `best` gives every
  a the b of its first edge;
* `rounds` restates the greedy as the device runs it: bids per b, then every row takes its largest
  live edge if it holds the bid, the rows in any order and seeing the matches made so far;
* `link_rows` .. `link` build the candidate rows of a source index in a target index from the oracle
  and reduce them.
"""
from __future__ import annotations

import numpy as np

import join_ref
import metric_ref
import sim_ref
import token_ref

NO_MATCH = 0xFFFFFFFF
INIT, BEGIN, BID, ACCEPT = 1, 2, 4, 8
TOKEN_SORT = 0x100


def order_bits(bits: int) -> int:
    """fp32 bits -> an unsigned int whose order is the floats' order, -0 below +0."""
    bits = int(bits) & 0xFFFFFFFF
    return (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits | 0x80000000


def block_rows(counts, keys, value_bits, n: int, stride: int, first: int, n_a: int, n_b: int) -> dict:
    """{a: [(order image of the value, b)]} of a block in ngsSearchDevice's layout: a count above the stride
    reads as the stride, an edge with a >= n_a or b >= n_b is ignored."""
    rows = {}
    for i in range(n):
        a = first + i
        if a >= n_a:
            continue
        c = min(int(counts[i]), stride)
        rows[a] = [(order_bits(value_bits[i * stride + r]), int(keys[i * stride + r])) for r in range(c)
                   if int(keys[i * stride + r]) < n_b]
    return rows


def greedy(n_a: int, n_b: int, rows: dict):
    """The sequential pass -> (match_a, match_b) lists."""
    edges = sorted((-v, a, b) for a, es in rows.items() for v, b in es)
    ma, mb = [NO_MATCH] * n_a, [NO_MATCH] * n_b
    for _, a, b in edges:
        if ma[a] == NO_MATCH and mb[b] == NO_MATCH:
            ma[a], mb[b] = b, a
    return ma, mb


def best(n_a: int, rows: dict):
    ma = [NO_MATCH] * n_a
    for a, es in rows.items():
        if es:
            ma[a] = min((-v, b) for v, b in es)[1]
    return ma


def one_round(rows: dict, ma, mb, rng=None) -> int:
    """One round in place -> the pairs it added. The bids come from the state at the round's start; the
    rows then accept in a shuffled order (rng) against the state as it is by then."""
    bids = {}
    for a, es in rows.items():
        if ma[a] != NO_MATCH:
            continue
        for v, b in es:
            if mb[b] == NO_MATCH and (b not in bids or bids[b] < (v, -a)):
                bids[b] = (v, -a)
    order = list(rows)
    if rng is not None:
        rng.shuffle(order)
    added = 0
    for a in order:
        if ma[a] != NO_MATCH:
            continue
        live = [(v, -b) for v, b in rows[a] if mb[b] == NO_MATCH]
        if not live:
            continue
        v, nb = max(live)
        if bids[-nb] == (v, -a):
            ma[a], mb[-nb] = -nb, a
            added += 1
    return added


def rounds(n_a: int, n_b: int, rows: dict, rng=None):
    """-> (match_a, match_b, rounds run, the last of which added nothing)."""
    ma, mb = [NO_MATCH] * n_a, [NO_MATCH] * n_b
    count = 0
    while True:
        count += 1
        if one_round(rows, ma, mb, rng) == 0:
            return ma, mb, count


# ---- the link of two indexes ----
def link_rows(oi_t, src_keys, omap_t, thr: float, limit: int):
    """rows[a] = (T key ids, fp32 score bits) as uint32 arrays: the oracle's full answer over T for the
    string of source key a, its ids mapped through omap_t, cut to min(limit, T's keys)."""
    ls = min(limit, len(omap_t))
    out = []
    for k, s in join_ref.oracle_full(oi_t, src_keys, thr):
        ids = omap_t[k].astype(np.uint32) if len(k) else k.astype(np.uint32)
        out.append((ids[:ls], s.view(np.uint32)[:ls]))
    return out


def row_sims(rows, src_keys, terms_t, metric: int, valid=sim_ref.DEFAULT_VALID, wide: bool = False):
    """The fp32 similarity bits of every record of `rows` (a uint32 array per row): the source key's raw
    string as the query, terms_t[b] the set of key b's terms as indexed; TOKEN_SORT in `metric` as the flag."""
    pairs = [(tuple(sim_ref.units(src_keys[a], wide)), terms_t[int(b)]) for a, (ids, _) in enumerate(rows) for b in ids]
    if metric & TOKEN_SORT:
        flat = token_ref.record_sims(pairs, metric & ~TOKEN_SORT, None, valid, wide)[0]
    else:
        flat = metric_ref.record_sims(pairs, metric, None, valid, wide)[0]
    out, at = [], 0
    for ids, _ in rows:
        out.append(flat[at:at + len(ids)].view(np.uint32).copy())
        at += len(ids)
    return out


def link(rows, n_t: int, sims=None, min_sim=None, one_to_one: bool = True):
    """-> (match, score bits, sim bits) uint32 arrays over the source keys, and the edges that were left.
    With sims (row_sims) and min_sim the records below it are dropped and the value is the similarity;
    otherwise the score. Unmatched: NO_MATCH, the bits of 0.0f and of -1.0f; without a filter every sim is -1.0f."""
    n_s = len(rows)
    filt = sims is not None and min_sim is not None and np.float32(min_sim) > np.float32(-1.0)
    edges = {}
    for a, (ids, sc) in enumerate(rows):
        es = []
        for r, b in enumerate(ids):
            if filt and np.uint32(sims[a][r]).view(np.float32) < np.float32(min_sim):
                continue
            es.append((order_bits(sims[a][r] if filt else sc[r]), int(b), r))
        edges[a] = es
    pairs = {a: [(v, b) for v, b, _ in es] for a, es in edges.items()}
    ma = greedy(n_s, n_t, pairs)[0] if one_to_one else best(n_s, pairs)
    minus_one = int(np.float32(-1.0).view(np.uint32))
    score = np.zeros(n_s, dtype=np.uint32)
    sim = np.full(n_s, minus_one, dtype=np.uint32)
    for a, b in enumerate(ma):
        if b == NO_MATCH:
            continue
        r = max((v, -r) for v, bb, r in edges[a] if bb == b)[1] * -1
        score[a] = rows[a][1][r]
        if filt:
            sim[a] = sims[a][r]
    return np.array(ma, dtype=np.uint32), score, sim, sum(len(es) for es in edges.values())
