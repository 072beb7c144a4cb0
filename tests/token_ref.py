"""Reference of the token sort and of the similarity with NGS_SIM_TOKEN_SORT (include/ngram_search.h,
"Token sort"), in Python and numpy alone, for tests/test_token_host.py and tests/test_gpu_token.py.
Strings are sequences of ints, as in sim_ref.

    token_sort(raw)      split at the separators, stable sort by the normalised tokens, join with single
                         blanks; the raw form keeps the raw characters and is padded with blanks to its
                         length, the stored form (a term as indexed) ends at L'
    record_sims(...)     metric_ref's DPs over Q' = normalise(token_sort(query)) and T' = the stored form
                         of every term; the matched term is the term as indexed
"""
from __future__ import annotations

import numpy as np

import metric_ref
import sim_ref
from sim_ref import DEFAULT_VALID, SIM_MAX_QUERY, SIM_NONE, SIM_WILDCARD

TOKEN_SORT = 0x100
BLANK = 32


def _runs(keep):
    """[(start, end)] of the maximal runs of True."""
    out, a = [], None
    for i, k in enumerate(keep):
        if k and a is None:
            a = i
        if not k and a is not None:
            out.append((a, i))
            a = None
    if a is not None:
        out.append((a, len(keep)))
    return out


def token_sort(raw, valid=DEFAULT_VALID, wide: bool = False, stored: bool = False) -> tuple:
    """The token-sorted form of `raw`: len(raw) characters in the raw form, L' <= len(raw) in the stored one."""
    raw = tuple(int(c) for c in raw)
    if stored:
        keep = [not sim_ref._space(c) for c in raw]
        norm = raw
    else:
        if len(raw) == 1 and raw[0] == ord("*"):  # the wildcard, whatever the validChar set says of '*'
            return raw
        vs = frozenset(valid)
        esc = [sim_ref._esc(c, vs, wide) for c in raw]
        keep = [not sim_ref._space(c) for c in esc]
        norm = [sim_ref._upper(c) for c in esc]
    runs = _runs(keep)
    if runs and runs[-1][1] - runs[0][0] > SIM_MAX_QUERY:
        return raw
    runs.sort(key=lambda r: tuple(norm[r[0]:r[1]]))  # (tuples compare as the rule says; list.sort is stable)
    out = []
    for n, (a, b) in enumerate(runs):
        if n:
            out.append(BLANK)
        out += raw[a:b]
    if not stored:
        out += [BLANK] * (len(raw) - len(out))
    return tuple(out)


def sorted_query(raw, valid=DEFAULT_VALID, wide: bool = False) -> tuple:
    """Q' as the similarity kernel reads it from the token-sorted bytes."""
    return sim_ref.normalise(token_sort(raw, valid, wide), valid, wide)


def sorted_term(t) -> tuple:
    return token_sort(t, stored=True)


def record_sims(pairs, metric: int, term_ids=None, valid=DEFAULT_VALID, wide: bool = False):
    """metric_ref.record_sims with the flag: pairs [(raw query, the key's terms as indexed, or None)] ->
    (float32 sims, matched terms as indexed or None each; the second value None without term_ids)."""
    out = np.full(len(pairs), SIM_NONE, dtype=np.float32)
    best = [None] * len(pairs)
    qn, tn = {}, {}
    jobs = []
    for r, (raw, terms) in enumerate(pairs):
        raw = tuple(raw)
        if sim_ref.is_wildcard(token_sort(raw, valid, wide)):
            out[r] = SIM_WILDCARD
            continue
        if terms is None:
            continue
        if raw not in qn:
            qn[raw] = sorted_query(raw, valid, wide)
        q = qn[raw]
        if len(q) > SIM_MAX_QUERY:
            continue
        for t in terms:
            if t not in tn:
                tn[t] = sorted_term(t)
            if len(tn[t]):
                jobs.append((q, tn[t], r, t))
    uniq = sorted({(q, ts) for q, ts, _, _ in jobs}, key=lambda p: (len(p[0]), len(p[1])))
    d = metric_ref.dist_batch([p[0] for p in uniq], [p[1] for p in uniq], metric) if uniq else []
    dmap = {p: int(x) for p, x in zip(uniq, d)}
    for q, ts, r, t in jobs:
        s = metric_ref.sim_value(dmap[(q, ts)], len(q), len(ts), metric)
        if best[r] is None or s > out[r] or (s == out[r] and term_ids is not None and term_ids[t] < term_ids[best[r]]):
            out[r] = s
            best[r] = t
    return out, (best if term_ids is not None else None)


def plain_sim(q, t, metric: int, valid=DEFAULT_VALID, wide: bool = False) -> np.float32:
    """sim(Q, T) of one raw query and one term as indexed, without the flag."""
    return metric_ref.record_sims([(tuple(q), {tuple(t)})], metric, None, valid, wide)[0][0]


def sorted_sim(q, t, metric: int, valid=DEFAULT_VALID, wide: bool = False) -> np.float32:
    """sim(Q', T') of the same pair."""
    return record_sims([(tuple(q), {tuple(t)})], metric, None, valid, wide)[0][0]


# ---- planted reordered pairs (shared by the CPU and the GPU tests) ---------------------------------
def reorder_pairs(rng, n: int, alpha=b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") -> list:
    """n (name, the name's words in another order) pairs of bytes: two or three distinct words of 4..7 letters."""
    out, seen = [], set()
    while len(out) < n:
        words = [bytes(rng.choice(alpha) for _ in range(rng.randint(4, 7))) for _ in range(rng.randint(2, 3))]
        if len(set(words)) < len(words):
            continue
        other = words[1:] + words[:1] if rng.random() < 0.5 else words[::-1]
        a, b = b" ".join(words), b" ".join(other)
        if a == b or a in seen or b in seen:
            continue
        seen |= {a, b}
        out.append((a, b))
    return out


def assert_reorder_matters(pairs, valid=DEFAULT_VALID):
    """On the model alone: sim(Q', T') > sim(Q, T) for every planted pair under Levenshtein and OSA, so
    an implementation that ignores the flag cannot pass."""
    for metric in (metric_ref.LEVENSHTEIN, metric_ref.OSA):
        for a, b in pairs:
            t = sim_ref.normalise(b, valid)
            s1, s0 = sorted_sim(a, t, metric, valid), plain_sim(a, t, metric, valid)
            assert s1 == np.float32(1.0) and s1 > s0, (a, b, metric, s1, s0)
