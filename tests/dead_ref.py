"""A numpy model of the dead-key row rule (stringsearchlib_amd/csrc/ngs_set.h: drop_dead_row, k_drop_dead)
and of the over-fetch loop of a set search with dead keys.

A block is a dict: n rows, stride, counts[n], keys[n * stride], scores[n * stride] (fp32 bits as u32),
n_keys and dead, the mask as u32 words (bit k & 31 of word k >> 5), or None with n_keys 0."""
from __future__ import annotations

import numpy as np

LIMIT_ALL = 2 ** 31 - 1
FETCH0 = 64      # kSetDeadFetch0
GROWTH = 4       # kSetDeadFetchGrowth
FAST_LIMIT = 128 # kSetDeadFastLimit: the search's one-wave tier takes limits up to it
FETCH_MIN = 16   # kSetDeadFetchMin


def mask(n_keys: int, dead_ids) -> np.ndarray:
    """The mask of `dead_ids` over n_keys keys: (n_keys + 31) // 32 words."""
    words = np.zeros((n_keys + 31) // 32, dtype=np.uint32)
    for k in dead_ids:
        assert 0 <= k < 32 * len(words)
        words[k >> 5] |= np.uint32(1 << (k & 31))
    return words


def is_dead(block, k: int) -> bool:
    return k < block["n_keys"] and bool((int(block["dead"][k >> 5]) >> (k & 31)) & 1)


def drop(block, limit: int):
    """-> (counts, rows, short rows): the row rule on every row; a row is [(key, score bits)]."""
    L = limit if limit else LIMIT_ALL
    stride, counts, rows, short = block["stride"], [], [], 0
    for i in range(block["n"]):
        c = min(int(block["counts"][i]), stride)
        at = i * stride
        live = [(int(k), int(s)) for k, s in zip(block["keys"][at:at + c], block["scores"][at:at + c])
                if not is_dead(block, int(k))]
        short += c == stride and len(live) < L
        rows.append(live[:L])
        counts.append(len(rows[-1]))
    return np.array(counts, dtype=np.uint32), rows, int(short)


def first_fetch(d: int, L: int) -> int:
    return min(d, FAST_LIMIT - L if L <= FAST_LIMIT - FETCH_MIN else max(L, FETCH0))


def fetch_stride(L: int, E: int, n_keys: int) -> int:
    return min(L + E, LIMIT_ALL, n_keys)


def over_fetch(hits, dead: set, n_keys: int, limit: int):
    """One member's row of a set search with dead keys: `hits` is the member's whole ranked hit list
    (local ids, what a search at limit 0 returns). -> (the row, the over-fetches E used)."""
    L = limit if limit else LIMIT_ALL
    d = len(dead)
    if d == 0:
        return list(hits[:min(L, n_keys)]), []
    E, used = first_fetch(d, L), []
    while True:
        used.append(E)
        stride = fetch_stride(L, E, n_keys)
        block = hits[:stride]
        live = [k for k in block if k not in dead]
        short = len(block) == stride and len(live) < L
        if not short or stride >= fetch_stride(L, d, n_keys):
            return live[:L], used
        E = min(d, E * GROWTH)
