"""A numpy model of the merge of result blocks (stringsearchlib_amd/csrc/ngs_set.h), and a
brute-force sort of tuples that the model is checked against.

A part is a dict: counts[n] u32, keys[n * stride] u32, scores[n * stride] u32 (fp32 bits), stride, base,
lens[n_keys] u32. merge() gives (counts[n], [row]) with a row the list of (key id, score bits)."""
from __future__ import annotations

import numpy as np

NO_LEN = 0xFFFFFFFF
LIMIT_ALL = 2**31 - 1


def order_bits(bits):
    """ngs_sim.h's sim_order_bits on u32 arrays: numeric order for non-NaN floats, -0 < +0."""
    b = np.asarray(bits, dtype=np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def min_stride(parts, limit: int) -> int:
    return min(limit or LIMIT_ALL, sum(int(p["stride"]) for p in parts))


def _row(parts, i):
    """Row i's records as columns: inverted order image, length, part, local id, global id, bits."""
    cols = [[] for _ in range(6)]
    for p, part in enumerate(parts):
        stride = int(part["stride"])
        c = min(int(part["counts"][i]), stride)
        k = part["keys"][i * stride:i * stride + c].astype(np.uint32)
        s = part["scores"][i * stride:i * stride + c].astype(np.uint32)
        lens = np.asarray(part["lens"], dtype=np.uint32)
        ln = np.full(c, NO_LEN, dtype=np.uint32)
        inside = k < len(lens)
        ln[inside] = lens[k[inside]]
        for col, v in zip(cols, (~order_bits(s), ln, np.full(c, p, dtype=np.uint32), k,
                                 (k + np.uint32(part["base"])).astype(np.uint32), s)):
            col.append(v)
    return [np.concatenate(c) if c else np.zeros(0, dtype=np.uint32) for c in cols]


def merge(parts, n: int, limit: int):
    """The numpy model: a lexsort of every row's union, cut to the limit."""
    L = limit or LIMIT_ALL
    counts, rows = np.zeros(n, dtype=np.uint32), []
    for i in range(n):
        inv, ln, p, k, g, s = _row(parts, i)
        order = np.lexsort((k, p, ln, inv))[:L]
        counts[i] = len(order)
        rows.append(list(zip(g[order].tolist(), s[order].tolist())))
    return counts, rows


def merge_brute(parts, n: int, limit: int):
    """The same by Python's sort of (order descending, length, part, id) tuples."""
    L = limit or LIMIT_ALL
    counts, rows = np.zeros(n, dtype=np.uint32), []
    for i in range(n):
        recs = []
        for p, part in enumerate(parts):
            stride = int(part["stride"])
            for r in range(min(int(part["counts"][i]), stride)):
                k, b = int(part["keys"][i * stride + r]), int(part["scores"][i * stride + r])
                img = (~b & 0xFFFFFFFF) if b & 0x80000000 else b | 0x80000000
                ln = int(part["lens"][k]) if k < len(part["lens"]) else NO_LEN
                recs.append((-img, ln, p, k, (k + int(part["base"])) & 0xFFFFFFFF, b))
        recs.sort()
        counts[i] = min(len(recs), L)
        rows.append([(g, b) for _, _, _, _, g, b in recs[:L]])
    return counts, rows
