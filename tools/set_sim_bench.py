#!/usr/bin/env python3
"""The similarity and the clusters over an index set against one index.

Workload: tools/set_bench.py's (a 1M-row library, no weights; a set of 4 equal parts; 4,096 queries at
threshold 0.3 and limit 100), one process, one GPU. Legs:
  (a) ngsSimilarityDeviceM on the one index's result block;
  (b) ngsSetSimilarityDeviceM on the set's block: the same records, by §9.7's exactness;
  (c) dedupKeysM on the one index;   (d) dedupKeysSet.
(a) and (b) are timed with HIP events on one stream, --reps samples each after a warm-up, alternating;
a sample is --launches calls back to back between the two events, divided by their number (one launch
of some twenty microseconds would measure the events as much as the kernel).
The workload's rows are short, so the two kernels are also timed on full rows: every query against
`limit` keys drawn at random from the whole library (other records for (a) and (b), of one
distribution). (c) and (d) are host calls that own their stream and return when the labels are back:
they are timed on the host clock around the call, alternating, until --dedup-reps samples or
--dedup-budget seconds. Prints one JSON line.

--legs a runs leg (a) alone through entry points older builds have as well (NGS_LIB=<name> selects
lib/libngram_search_<name>.so): the check that the single-index kernel did not move.

    python tools/set_sim_bench.py [--rows 1000000] [--reps 50] [--legs abcd]
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

PARTS = 4
OSA = 1


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def note(msg):
    print(f"[set_sim_bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--threshold", type=float, default=0.3)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--dedup-reps", type=int, default=50)
    ap.add_argument("--dedup-budget", type=float, default=0.0, help="seconds for legs (c) and (d); 0: no bound")
    ap.add_argument("--dedup-limit", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("set_sim_bench: no GPU")
    L = _native.lib()
    with_set = bool(set(a.legs) & set("bd"))
    corpus = Corpus(a.rows)
    whole = build_index(corpus, False, 0)
    members, sid = [], 0
    if with_set:
        cuts = [a.rows * p // PARTS for p in range(PARTS + 1)]
        words = C.cast(corpus.words, C.c_void_p).value
        for lo, hi in zip(cuts, cuts[1:]):
            h = L.indexN(C.cast(words + 8 * lo, C.POINTER(C.c_char_p)), hi - lo, 1, None)
            if not h:
                raise SystemExit("set_sim_bench: indexN of a part failed")
            members.append(h)
        sid = L.ngsSetCreate((C.c_uint32 * PARTS)(*members), PARTS)
        if not sid:
            raise SystemExit(f"set_sim_bench: ngsSetCreate failed ({L.ngsLastError(1)})")
    nk = L.ngsNumKeys(whole)
    note(f"{nk} keys indexed")

    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    s = st.cuda_stream
    B, lim, thr = a.queries, a.limit, a.threshold
    raw, offs = corpus.queries(B)
    d_raw = torch.from_numpy(np.frombuffer(raw + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    q = (d_raw.data_ptr(), d_off.data_ptr(), B)

    def block():
        return (torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B * lim, dtype=torch.int32, device=dev),
                torch.zeros(B * lim, dtype=torch.float32, device=dev))

    one, merged = block(), block()
    sim_one, sim_set = (torch.zeros(B * lim, dtype=torch.float32, device=dev) for _ in range(2))
    if L.ngsSearchDevice(whole, *q, thr, lim, lim, *[t.data_ptr() for t in one], s):
        raise SystemExit("set_sim_bench: the search failed")
    if with_set and L.ngsSetSearchDevice(sid, *q, thr, lim, lim, *[t.data_ptr() for t in merged], s):
        raise SystemExit("set_sim_bench: the set search failed")
    # full rows: `limit` random keys a query
    g = torch.Generator(device="cpu").manual_seed(7)
    full_n = torch.full((B,), lim, dtype=torch.int32, device=dev)
    ids = min(nk, L.ngsSetNumKeys(sid)) if with_set else nk
    full_k = torch.randint(0, ids, (B * lim,), generator=g).int().to(dev)
    sim_full = torch.zeros(B * lim, dtype=torch.float32, device=dev)
    st.synchronize()
    torch.cuda.synchronize()

    legs = {}
    if "a" in a.legs:
        legs["one_index_sim_ms"] = lambda: L.ngsSimilarityDeviceM(whole, *q, lim, one[0].data_ptr(), one[1].data_ptr(), OSA,
                                                                  sim_one.data_ptr(), None, s)
        legs["one_index_sim_full_rows_ms"] = lambda: L.ngsSimilarityDeviceM(
            whole, *q, lim, full_n.data_ptr(), full_k.data_ptr(), OSA, sim_full.data_ptr(), None, s)
    if "b" in a.legs:
        legs["set_sim_ms"] = lambda: L.ngsSetSimilarityDeviceM(sid, *q, lim, merged[0].data_ptr(), merged[1].data_ptr(), OSA,
                                                               sim_set.data_ptr(), None, s)
        legs["set_sim_full_rows_ms"] = lambda: L.ngsSetSimilarityDeviceM(
            sid, *q, lim, full_n.data_ptr(), full_k.data_ptr(), OSA, sim_full.data_ptr(), None, s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        for _ in range(a.launches):
            if fn():
                raise SystemExit("set_sim_bench: a call failed")
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1) / a.launches

    for fn in legs.values():  # warm-up of each (the first call builds the key -> term maps)
        for _ in range(3):
            timed(fn)
    times = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    note("similarity legs done")
    out = {"rows": a.rows, "parts": PARTS, "queries": B, "threshold": thr, "limit": lim, "metric": "osa", "keys": nk,
           "reps": a.reps, "launches_per_sample": a.launches,
           "records": int(one[0].sum().item()), **{k: spread(v) for k, v in times.items()}}
    if "a" in a.legs and "b" in a.legs:
        n1, n2 = one[0].cpu().numpy(), merged[0].cpu().numpy()
        live = (np.arange(lim)[None, :] < n1[:, None]).reshape(-1)
        out["set_sims_equal_one_index"] = bool(np.array_equal(n1, n2) and np.array_equal(
            sim_one.cpu().numpy().view(np.uint32)[live], sim_set.cpu().numpy().view(np.uint32)[live]))
        med = lambda k: statistics.median(times[k])
        out["set_over_one_index_sim"] = round(med("set_sim_ms") / med("one_index_sim_ms"), 4)
        out["set_over_one_index_sim_full_rows"] = round(med("set_sim_full_rows_ms") / med("one_index_sim_full_rows_ms"), 4)

    dedup = {}
    if "c" in a.legs:
        lab_one = np.zeros(nk, dtype=np.uint32)
        dedup["dedup_one_index_ms"] = lambda: L.dedupKeysM(whole, thr, a.dedup_limit, OSA, 0.8, 0,
                                                           lab_one.ctypes.data_as(C.POINTER(C.c_uint32)))
    if "d" in a.legs:
        lab_set = np.zeros(nk, dtype=np.uint32)
        dedup["dedup_set_ms"] = lambda: L.dedupKeysSet(sid, thr, a.dedup_limit, OSA, 0.8, 0,
                                                       lab_set.ctypes.data_as(C.POINTER(C.c_uint32)))
    if dedup:
        clusters, dtimes = {}, {k: [] for k in dedup}
        for k, fn in dedup.items():  # warm-up
            clusters[k] = fn()
            if not clusters[k]:
                raise SystemExit(f"set_sim_bench: {k} failed ({L.ngsLastError(1)})")
        t_end = time.perf_counter() + a.dedup_budget if a.dedup_budget else float("inf")
        while len(next(iter(dtimes.values()))) < a.dedup_reps and time.perf_counter() < t_end:
            for k, fn in dedup.items():
                t0 = time.perf_counter()
                if fn() != clusters[k]:
                    raise SystemExit(f"set_sim_bench: {k} is not reproducible")
                dtimes[k].append((time.perf_counter() - t0) * 1e3)
            note(f"dedup sample {len(next(iter(dtimes.values())))}")
        out.update({k: spread(v) for k, v in dtimes.items()})
        out["dedup"] = {"limit": a.dedup_limit, "min_similarity": 0.8, "clusters": clusters}
        if len(dedup) == 2:
            out["dedup_cluster_counts_equal"] = clusters["dedup_one_index_ms"] == clusters["dedup_set_ms"]
            out["set_over_one_index_dedup"] = round(statistics.median(dtimes["dedup_set_ms"]) /
                                                    statistics.median(dtimes["dedup_one_index_ms"]), 4)
    out["version"] = L.ngsVersion().decode()
    print(json.dumps(out))
    if sid:
        L.ngsSetDispose(sid)
    for h in members + [whole]:
        L.dispose(h)


if __name__ == "__main__":
    main()
