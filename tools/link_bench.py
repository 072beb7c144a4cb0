#!/usr/bin/env python3
"""Linking two libraries on the device, against the route a caller had without linkKeys.

Workload: T is bench C2's corpus (--rows rows, no weights); S has as many words, half of them
single-substitution variants of keys of T, half unrelated synthetic words. Threshold 0.5, limit 10,
Levenshtein similarity at least 0.85, one process, one GPU.
  new  linkKeys, NGS_LINK_BEST and NGS_LINK_ONE_TO_ONE (each call ends synchronised);
  old  the strings of S's keys (ngsKey; the pointers are fetched once, outside the timing),
       scoreBatchSimM on T in calls of 65,536 queries, the records' key ids from their result pointers,
       then on the host a numpy sort of all edges by (similarity descending, a, b) and one sequential
       scan that takes an edge when both its ends are free (the best record of a key is its first edge
       in that order).
Both routes run alternately, --reps times each after one warm-up of each; wall clock around each, the
median with the smallest and largest as the spread; then the two linkKeys calls again, each --reps
times one after the other (a call that follows the host route's host work is slower than one that
follows another call). The matches of the two routes are compared at full size, in both modes.
Then, in the same process, the device composition the header documents, timed with HIP events on one
stream: the candidate block (ngsKeyQueriesDevice on S, ngsSearchDevice and ngsRerankDeviceM on T, a
batch at a time into one block) and the rounds of ngsMatchDevice over it, the pair count read between
rounds: the number of rounds, each round's pairs, and the rounds' share of block + rounds.
Prints one JSON line.

    python tools/link_bench.py [--rows 1000000] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process: torch's first)

from bench import Corpus, build_index  # noqa: E402
from stringsearchlib_amd import _native  # noqa: E402
from stringsearchlib_amd.synth import ALPHABET  # noqa: E402

BATCH = 65536
NO_MATCH = 0xFFFFFFFF


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def order_image(sim):
    """fp32 -> uint32 whose order is the floats' order (the edge order's image of a value)."""
    b = sim.view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def greedy_host(a, b, sim, n_s, n_t):
    """The host route's reduction: (best, one-to-one) match arrays from flat edges."""
    order = np.lexsort((b, a, ~order_image(sim)))  # value descending, then a, then b
    a, b = a[order], b[order]
    best = np.full(n_s, NO_MATCH, dtype=np.uint32)
    first = np.unique(a, return_index=True)[1]     # a's first edge in the order
    best[a[first]] = b[first]
    one = np.full(n_s, NO_MATCH, dtype=np.uint32)
    taken = np.zeros(n_t, dtype=bool)
    for x, y in zip(a.tolist(), b.tolist()):       # the sequential scan
        if one[x] == NO_MATCH and not taken[y]:
            one[x] = y
            taken[y] = True
    return best, one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--min-similarity", type=float, default=0.85)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("link_bench: no GPU")
    L = _native.lib()
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    lim, thr, ms = a.limit, a.threshold, a.min_similarity

    # T, and S: variants of T's keys and unrelated words, shuffled
    ct = Corpus(a.rows)
    ht = build_index(ct, False, 0)
    nt = L.ngsNumKeys(ht)
    tptr = np.array([L.ngsKey(ht, k) for k in range(nt)], dtype=np.uint64)  # ascending with k
    assert (np.diff(tptr.astype(np.int64)) > 0).all()
    rng = random.Random(7)
    words = []
    for k in rng.choices(range(nt), k=a.rows // 2):  # with replacement: some keys of T get several variants
        w = bytearray(C.string_at(int(tptr[k])))
        w[rng.randrange(len(w))] = rng.choice(ALPHABET)
        words.append(bytes(w))
    other = Corpus(a.rows - len(words), seed=4242)
    words += [other.words[i] for i in range(other.n_words)]
    other.free()
    rng.shuffle(words)
    arr = (C.c_char_p * len(words))(*words)
    hs = L.indexN(arr, len(words), 1, None)
    if not hs:
        raise SystemExit("link_bench: indexN of the source failed")
    ns = L.ngsNumKeys(hs)
    sptr = np.array([L.ngsKey(hs, k) for k in range(ns)], dtype=np.uint64)
    assert (np.diff(sptr.astype(np.int64)) > 0).all()
    qarr = (C.c_char_p * ns).from_buffer(sptr.view(np.int64))

    def new_route(mode):
        match = np.zeros(ns, dtype=np.uint32)
        L.ngsLastError(1)
        t = time.perf_counter()
        n = L.linkKeys(hs, ht, thr, lim, 0, ms, mode, 0, match.ctypes.data_as(u32p), None, None)
        dt = time.perf_counter() - t
        if L.ngsLastError(1) or n != int((match != NO_MATCH).sum()):
            raise SystemExit("link_bench: linkKeys failed")
        return dt, match

    def old_route():
        t = time.perf_counter()
        ea, eb, ev = [], [], []
        for a0 in range(0, ns, BATCH):
            n = min(BATCH, ns - a0)
            cnt = np.zeros(n, dtype=np.uint32)
            res, sc, sv = C.POINTER(C.POINTER(C.c_char))(), f32p(), f32p()
            qs = C.cast(C.addressof(qarr) + a0 * 8, C.POINTER(C.c_char_p))
            total = L.scoreBatchSimM(ht, qs, n, thr, lim, 0, ms, cnt.ctypes.data_as(u32p), C.byref(res), C.byref(sc),
                                     C.byref(sv), None)
            if total:
                rp = np.ctypeslib.as_array(C.cast(res, C.POINTER(C.c_uint64)), (total,))
                ea.append(np.repeat(np.arange(a0, a0 + n, dtype=np.uint32), cnt))
                eb.append(np.searchsorted(tptr, rp).astype(np.uint32))
                ev.append(np.ctypeslib.as_array(sv, (total,)).copy())
            if res:
                L.release(ht, res, sc)
            # (the similarities are a new[]'d float array like the scores: release() frees one such array)
            if sv:
                L.release(ht, None, sv)
        t_batches = time.perf_counter() - t
        e = [np.concatenate(x) if x else np.zeros(0, dtype=d) for x, d in ((ea, np.uint32), (eb, np.uint32),
                                                                             (ev, np.float32))]
        best, one = greedy_host(e[0], e[1], e[2], ns, nt)
        dt = time.perf_counter() - t
        return dt, t_batches, best, one, len(e[0])

    new_route(0), new_route(1), old_route()  # warm-up
    t_best, t_one, t_old, t_old_batches = [], [], [], []
    for _ in range(a.reps):
        d0, m0 = new_route(0)
        d1, m1 = new_route(1)
        do, db, ob, oo, edges = old_route()
        t_best.append(d0), t_one.append(d1), t_old.append(do), t_old_batches.append(db)
    same = bool((m0 == ob).all() and (m1 == oo).all())
    # the same calls one after the other, without the host route's half second of host work between them
    t_best_b2b = [new_route(0)[0] for _ in range(a.reps + 1)][1:]
    t_one_b2b = [new_route(1)[0] for _ in range(a.reps + 1)][1:]

    # ---- the device composition: the block, then the rounds, on one stream ----
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    s = st.cuda_stream
    ls = min(lim, nt)
    nb = min(BATCH, ns)
    raw = torch.zeros(max(L.ngsKeyQueryBytes(hs, a0, min(nb, ns - a0)) for a0 in range(0, ns, nb)) + 16,
                      dtype=torch.uint8, device=dev)
    off = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    dn = torch.zeros(ns, dtype=torch.int32, device=dev)
    dk = torch.zeros(ns * ls, dtype=torch.int32, device=dev)
    ds = torch.zeros(ns * ls, dtype=torch.float32, device=dev)
    dv = torch.zeros(ns * ls, dtype=torch.float32, device=dev)
    ma = torch.zeros(ns, dtype=torch.int32, device=dev)
    mb = torch.zeros(nt, dtype=torch.int32, device=dev)
    bids = torch.zeros(nt, dtype=torch.int64, device=dev)
    matched = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def block():
        for a0 in range(0, ns, nb):
            n = min(nb, ns - a0)
            rc = L.ngsKeyQueriesDevice(hs, a0, n, raw.data_ptr(), raw.numel() - 16, off.data_ptr(), s)
            rc = rc or L.ngsSearchDevice(ht, raw.data_ptr(), off.data_ptr(), n, thr, lim, ls, dn.data_ptr() + 4 * a0,
                                         dk.data_ptr() + 4 * a0 * ls, ds.data_ptr() + 4 * a0 * ls, s)
            rc = rc or L.ngsRerankDeviceM(ht, raw.data_ptr(), off.data_ptr(), n, ls, dn.data_ptr() + 4 * a0,
                                          dk.data_ptr() + 4 * a0 * ls, ds.data_ptr() + 4 * a0 * ls,
                                          dv.data_ptr() + 4 * a0 * ls, None, 0, ms, s)
            if rc:
                raise SystemExit(f"link_bench: the block failed: {rc}")

    def rounds():
        adds, before, flags = [], 0, 15
        while True:
            if L.ngsMatchDevice(dn.data_ptr(), dk.data_ptr(), dv.data_ptr(), ns, ls, 0, ma.data_ptr(), ns, mb.data_ptr(),
                                nt, bids.data_ptr(), matched.data_ptr(), flags, s):
                raise SystemExit("link_bench: ngsMatchDevice failed")
            flags = 14
            st.synchronize()
            now = int(matched.cpu().numpy()[0])
            adds.append(now - before)
            before = now
            if adds[-1] == 0:
                return adds

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        out = fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1), out

    t_block, t_rounds, adds = [], [], []
    for _ in range(a.reps + 1):
        tb, _ = timed(block)
        tr, adds = timed(rounds)
        t_block.append(tb), t_rounds.append(tr)
    t_block, t_rounds = spread(t_block[1:]), spread(t_rounds[1:])
    composed = ma.cpu().numpy().view(np.uint32)
    same_composed = bool((composed == m1).all())
    print(json.dumps({
        "rows": a.rows, "source_keys": ns, "target_keys": nt, "threshold": thr, "limit": lim, "metric": "levenshtein",
        "min_similarity": ms, "reps": a.reps,
        "linkKeys_best_s": spread(t_best), "linkKeys_one_to_one_s": spread(t_one),
        "linkKeys_best_back_to_back_s": spread(t_best_b2b), "linkKeys_one_to_one_back_to_back_s": spread(t_one_b2b),
        "host_route_s": spread(t_old), "host_route_scoreBatchSimM_s": spread(t_old_batches),
        "ratio_one_to_one_over_host_route": round(statistics.median(t_one) / statistics.median(t_old), 4),
        "edges": int(edges), "matched_best": int((m0 != NO_MATCH).sum()), "matched_one_to_one": int((m1 != NO_MATCH).sum()),
        "differ_best_vs_one_to_one": int((m0 != m1).sum()), "matches_equal": same,
        "device_block_ms": t_block, "device_rounds_ms": t_rounds, "rounds": len(adds), "pairs_per_round": adds[:16],
        "rounds_share_of_block_plus_rounds": round(t_rounds["median"] / (t_rounds["median"] + t_block["median"]), 4),
        "device_composition_equal": same_composed,
        "block_bytes": int(ns) * ls * 12 + int(ns) * 4, "version": L.ngsVersion().decode()}))
    if not (same and same_composed):
        raise SystemExit("link_bench: the routes' matches differ")
    L.dispose(hs)
    L.dispose(ht)
    ct.free()


if __name__ == "__main__":
    main()
