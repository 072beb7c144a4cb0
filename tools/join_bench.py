#!/usr/bin/env python3
"""The self-join of a whole library, against the route a caller had without it.

Workload: bench C2's corpus (1M rows, no weights), threshold 0.5, limit 10, one process, one GPU.
  new  selfJoin of the whole library into caller-allocated arrays (the call ends synchronised);
  old  the key strings (ngsKey; the pointers are fetched once, outside the timing), scoreBatch at
       limit 11 in calls of 65,536 queries, the key's own record dropped and the row cut to 10 on
       the host (numpy, vectorised), into arrays of the same layout.
Both routes run alternately, --reps times each after one warm-up of each; wall clock around each, the
median with the smallest and largest as the spread. The two record sets are compared at full size.
Then, in the same process, the stages' own times from HIP events on one stream (median of --reps):
the gather of a 65,536-key batch, drop-self on that batch's search output, and ngsClusterDevice over
the whole join's records (init, unions and finish apart), the unions and the finish against the
bytes they must move at the least (counts, records and labels x 4; labels x 8) as a share of --hbm-peak;
and the same two passes over a fabricated full block (every row with `limit` partners at most 64 ids
away: one component), the rate of the union-find when every cell is an edge.
Prints one JSON line.

    python tools/join_bench.py [--rows 1000000] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process: torch's first)

from bench import Corpus, build_index  # noqa: E402
from stringsearchlib_amd import _native  # noqa: E402

BATCH = 65536


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def drop_self_host(rp, cnt, self_ptr, lim):
    """The old route's host step on one scoreBatch answer: rp the flat result pointers, cnt the rows'
    counts, self_ptr each row's own key pointer. -> (row, place in the row, mask) of the records kept:
    the key's own record dropped, the others moved up, the row cut to lim."""
    cnt = cnt.astype(np.int64)
    row = np.repeat(np.arange(len(cnt)), cnt)
    keep = rp != self_ptr[row]
    start = np.cumsum(cnt) - cnt                     # each row's first record
    ck = np.cumsum(keep)
    rank = ck - 1 - (ck[start[row]] - keep[start[row]])  # kept records before this one in its row
    keep &= rank < lim
    return row[keep], rank[keep], keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes/s the shares are quoted against")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("join_bench: no GPU")
    L = _native.lib()
    corpus = Corpus(a.rows)
    h = build_index(corpus, False, 0)
    nk, lim = L.ngsNumKeys(h), a.limit
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)

    def new_route():
        counts = np.zeros(nk, dtype=np.uint32)
        keys = np.zeros((nk, lim), dtype=np.uint32)
        scores = np.zeros((nk, lim), dtype=np.float32)
        L.ngsLastError(1)
        t = time.perf_counter()
        total = L.selfJoin(h, 0, nk, a.threshold, lim, lim, counts.ctypes.data_as(u32p), keys.ctypes.data_as(u32p),
                           scores.ctypes.data_as(f32p))
        dt = time.perf_counter() - t
        if total != int(counts.sum()) or L.ngsLastError(1):
            raise SystemExit("join_bench: selfJoin failed")
        return dt, counts, keys, scores

    kptr = np.array([L.ngsKey(h, k) for k in range(nk)], dtype=np.uint64)  # ascending with k
    assert (np.diff(kptr.astype(np.int64)) > 0).all()
    qarr = (C.c_char_p * nk).from_buffer(kptr.view(np.int64))

    def old_route():
        counts = np.zeros(nk, dtype=np.uint32)
        keys = np.zeros((nk, lim), dtype=np.uint32)
        scores = np.zeros((nk, lim), dtype=np.float32)
        t = time.perf_counter()
        for a0 in range(0, nk, BATCH):
            n = min(BATCH, nk - a0)
            cnt = np.zeros(n, dtype=np.uint32)
            res, sc = C.POINTER(C.POINTER(C.c_char))(), f32p()
            qs = C.cast(C.addressof(qarr) + a0 * 8, C.POINTER(C.c_char_p))
            total = L.scoreBatch(h, qs, n, a.threshold, lim + 1, cnt.ctypes.data_as(u32p), C.byref(res), C.byref(sc))
            if total:
                rp = np.ctypeslib.as_array(C.cast(res, C.POINTER(C.c_uint64)), (total,))
                rs = np.ctypeslib.as_array(sc, (total,))
                r, c, keep = drop_self_host(rp, cnt, kptr[a0:a0 + n], lim)
                keys[a0 + r, c] = np.searchsorted(kptr, rp[keep])
                scores[a0 + r, c] = rs[keep]
                counts[a0:a0 + n] = np.bincount(r, minlength=n)
            if res:
                L.release(h, res, sc)
        return time.perf_counter() - t, counts, keys, scores

    new_route(), old_route()  # warm-up
    t_new, t_old = [], []
    for _ in range(a.reps):
        dn_, cn, kn, sn = new_route()
        do_, co, ko, so = old_route()
        t_new.append(dn_)
        t_old.append(do_)
    live = np.arange(lim)[None, :] < cn[:, None]
    same = bool((cn == co).all() and (kn[live] == ko[live]).all() and
                (sn.view(np.uint32)[live] == so.view(np.uint32)[live]).all())
    records = int(cn.sum())

    # ---- the stages' own times ----
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()

    def timed(fn, before=None):
        out = []
        for _ in range(a.reps + 1):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.synchronize()
            e0.record(st)
            if fn():
                raise SystemExit("join_bench: a stage failed")
            e1.record(st)
            st.synchronize()
            out.append(e0.elapsed_time(e1))
        return spread(out[1:])

    n = min(BATCH, nk)
    qbytes = L.ngsKeyQueryBytes(h, 0, n)
    raw = torch.zeros(qbytes + 16, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    stride = lim + 1
    dn = torch.zeros(n, dtype=torch.int32, device=dev)
    dk = torch.zeros(n * stride, dtype=torch.int32, device=dev)
    ds = torch.zeros(n * stride, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    s = st.cuda_stream
    t_gather = timed(lambda: L.ngsKeyQueriesDevice(h, 0, n, raw.data_ptr(), qbytes, off.data_ptr(), s))
    if L.ngsSearchDevice(h, raw.data_ptr(), off.data_ptr(), n, a.threshold, stride, stride, dn.data_ptr(),
                         dk.data_ptr(), ds.data_ptr(), s):
        raise SystemExit("join_bench: ngsSearchDevice failed")
    keep_n, keep_k, keep_s = dn.clone(), dk.clone(), ds.clone()
    torch.cuda.synchronize()

    def restore():
        with torch.cuda.stream(st):
            dn.copy_(keep_n), dk.copy_(keep_k), ds.copy_(keep_s)
    t_drop = timed(lambda: L.ngsDropSelfDevice(dn.data_ptr(), dk.data_ptr(), ds.data_ptr(), n, stride, 0, lim, s),
                   restore)
    ec = torch.from_numpy(cn.view(np.int32)).to(dev)
    ek = torch.from_numpy(kn.view(np.int32).reshape(-1)).to(dev)
    lab = torch.zeros(nk, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    cl = lambda rows, flags: L.ngsClusterDevice(ec.data_ptr(), ek.data_ptr(), rows, lim, 0, lab.data_ptr(), nk, flags, s)
    t_init = timed(lambda: cl(0, 1))
    t_union = timed(lambda: cl(nk, 0), lambda: cl(0, 1))
    t_finish = timed(lambda: cl(0, 2), lambda: cl(nk, 1))
    clusters = int((lab.cpu().numpy().view(np.uint32) == np.arange(nk, dtype=np.uint32)).sum())
    # the same passes over a full block: every row with `lim` partners at most 64 ids away (one
    # component; the rate the kernel has when every cell is an edge)
    rng = np.random.default_rng(7)
    dense = ((np.arange(nk, dtype=np.int64)[:, None] + rng.integers(1, 65, (nk, lim))) % nk).astype(np.uint32)
    ek = torch.from_numpy(dense.view(np.int32).reshape(-1)).to(dev)
    ec = torch.full((nk,), lim, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t_union_dense = timed(lambda: cl(nk, 0), lambda: cl(0, 1))
    t_finish_dense = timed(lambda: cl(0, 2), lambda: cl(nk, 1))
    dense_clusters = int((lab.cpu().numpy().view(np.uint32) == np.arange(nk, dtype=np.uint32)).sum())
    dense_bytes = nk * 4 + nk * lim * 4 + nk * 4
    # the bytes a pass must move at the least: the unions read every row's count, every record's key
    # and a label per key; the finish reads and writes every label
    union_bytes = nk * 4 + records * 4 + nk * 4
    finish_bytes = nk * 4 + nk * 4
    share = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / a.hbm_peak, 5)
    print(json.dumps({
        "rows": a.rows, "keys": nk, "threshold": a.threshold, "limit": lim, "reps": a.reps,
        "selfJoin_s": spread(t_new), "scoreBatch_route_s": spread(t_old),
        "ratio_new_over_old": round(statistics.median(t_new) / statistics.median(t_old), 4),
        "records": records, "record_sets_equal": same,
        "gather_ms": t_gather, "gather_keys": n, "gather_bytes": int(qbytes),
        "drop_self_ms": t_drop, "drop_self_rows": n, "drop_self_stride": stride,
        "cluster_init_ms": t_init, "cluster_union_ms": t_union, "cluster_finish_ms": t_finish,
        "cluster_edges_cells": nk * lim, "cluster_labels": nk, "clusters": clusters,
        "union_least_bytes": union_bytes, "finish_least_bytes": finish_bytes, "hbm_peak_Bps": a.hbm_peak,
        "union_share_of_hbm_peak": share(union_bytes, t_union["median"]),
        "finish_share_of_hbm_peak": share(finish_bytes, t_finish["median"]),
        "dense_union_ms": t_union_dense, "dense_finish_ms": t_finish_dense, "dense_edges": nk * lim,
        "dense_clusters": dense_clusters, "dense_union_least_bytes": dense_bytes,
        "dense_union_share_of_hbm_peak": share(dense_bytes, t_union_dense["median"]),
        "version": L.ngsVersion().decode()}))
    if not same:
        raise SystemExit("join_bench: the two routes' record sets differ")
    L.dispose(h)


if __name__ == "__main__":
    main()
