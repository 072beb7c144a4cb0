#!/usr/bin/env python3
"""The cost of the similarity / re-rank stage behind the search.

A 200,000-row synthetic library (stringsearchlib_amd.synth, one key per row), 4,096 queries of 12
bytes cut from its keys with one substitution, threshold 0.3, limit 100, one process, one stream.
ngsSearchDevice alone and ngsSearchDevice with ngsRerankDevice queued behind it are timed
alternately: host clock from before the call to the end of a stream synchronise, 10 warm-ups of
each, the median of --reps calls with the 10th / 90th percentiles as the spread. The stage's own
time comes from HIP events around ngsRerankDevice (and around ngsSimilarityDevice alone) on the
same stream. Records and term characters are counted on the host from the search's answer.
--metric NAME (repeatable; "levenshtein", "osa" or "partial") times the same stage through
ngsRerankDeviceM / ngsSimilarityDeviceM by that metric as well, alternating with the stage above
within every repetition; --terms has those calls write the matched term ids too.
--token-sort times, besides all that, ngsTokenSortDevice alone (out of place, HIP events) and the
stage with NGS_SIM_TOKEN_SORT (the token sort of the batch and the flagged re-rank behind it) for
Levenshtein and every --metric, alternating with the unflagged stages; the first flagged call, which
builds the replica's token-sorted terms, is timed on the host clock and the arrays' bytes are
computed from the library.
Prints one JSON line.

    python tools/sim_probe.py [--rows 200000] [--queries 4096] [--reps 30] [--metric osa --metric partial] [--terms]
                              [--token-sort]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process: torch's first)

import sim_ref  # noqa: E402
import token_ref  # noqa: E402
import stringsearchlib_amd as ssl  # noqa: E402
from stringsearchlib_amd import _native  # noqa: E402

SECTOR = 64  # bytes a random access fetches at the least


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def spread(v):
    return {"median": round(statistics.median(v), 4), "p10": round(pct(v, 0.1), 4), "p90": round(pct(v, 0.9), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=0.3)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--min-similarity", type=float, default=0.0)
    ap.add_argument("--metric", action="append", default=[], choices=sorted(ssl.METRICS))
    ap.add_argument("--terms", action="store_true")
    ap.add_argument("--token-sort", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sim_probe: no GPU")
    words, weights, rng = ssl.synth.gen_corpus(a.rows, seed=42)
    queries = ssl.synth.gen_queries(words, 1, a.queries, rng)
    ix = ssl.StringIndex(words, 1, weights, device=0)
    nq, stride = len(queries), min(a.limit, ix.num_keys())
    dev = torch.device("cuda:0")
    offs = np.cumsum([0] + [len(q) for q in queries], dtype=np.int64)
    raw = torch.frombuffer(bytearray(b"".join(queries) + bytes(16)), dtype=torch.uint8).to(dev)
    off = torch.from_numpy(offs).to(dev)
    dn = torch.zeros(nq, dtype=torch.int32, device=dev)
    dk = torch.zeros(nq * stride, dtype=torch.int32, device=dev)
    ds = torch.zeros(nq * stride, dtype=torch.float32, device=dev)
    dv = torch.zeros(nq * stride, dtype=torch.float32, device=dev)
    dt = torch.zeros(nq * stride, dtype=torch.int32, device=dev)
    d_terms = dt.data_ptr() if a.terms else 0
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    args = (raw.data_ptr(), off.data_ptr(), nq)
    outs = (dn.data_ptr(), dk.data_ptr(), ds.data_ptr())

    def search():
        t = time.perf_counter()
        ix.search_device(*args, a.threshold, a.limit, stride, *outs, st.cuda_stream)
        st.synchronize()
        return (time.perf_counter() - t) * 1e3

    def search_rerank(metric=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        ix.search_device(*args, a.threshold, a.limit, stride, *outs, st.cuda_stream)
        e0.record(st)
        if metric is None:
            ix.rerank_device(*args, stride, *outs, dv.data_ptr(), a.min_similarity, st.cuda_stream)
        else:
            ix.rerank_device(*args, stride, *outs, dv.data_ptr(), a.min_similarity, st.cuda_stream, metric=metric,
                             d_terms=d_terms)
        e1.record(st)
        st.synchronize()
        return (time.perf_counter() - t) * 1e3, e0.elapsed_time(e1)

    def similarity_alone(metric=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        if metric is None:
            ix.similarity_device(*args, stride, dn.data_ptr(), dk.data_ptr(), dv.data_ptr(), st.cuda_stream)
        else:
            ix.similarity_device(*args, stride, dn.data_ptr(), dk.data_ptr(), dv.data_ptr(), st.cuda_stream,
                                 metric=metric, d_terms=d_terms)
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1)

    raw2 = torch.zeros_like(raw)  # the token-sorted batch: the search keeps reading the queries as they are

    def sort_alone():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        ix.token_sort_device(*args, raw2.data_ptr(), st.cuda_stream)
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1)

    def search_sorted_rerank(metric):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ix.search_device(*args, a.threshold, a.limit, stride, *outs, st.cuda_stream)
        e0.record(st)
        ix.token_sort_device(*args, raw2.data_ptr(), st.cuda_stream)
        ix.rerank_device(raw2.data_ptr(), off.data_ptr(), nq, stride, *outs, dv.data_ptr(), a.min_similarity,
                         st.cuda_stream, metric=metric, d_terms=d_terms, token_sort=True)
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1)

    flagged = ["levenshtein"] + [mt for mt in a.metric if mt != "levenshtein"] if a.token_sort else []
    build_ms = None
    if a.token_sort:  # the first flagged call on the replica builds its token-sorted terms (no records yet: dn is zero)
        t = time.perf_counter()
        ix.similarity_device(*args, stride, dn.data_ptr(), dk.data_ptr(), dv.data_ptr(), st.cuda_stream, token_sort=True)
        st.synchronize()
        build_ms = (time.perf_counter() - t) * 1e3
    for _ in range(a.warmup):
        search()
        search_rerank()
        for mt in a.metric:
            search_rerank(mt)
        for mt in flagged:
            search_sorted_rerank(mt)
    t_search, t_both, t_stage, t_sim = [], [], [], []
    m_stage, m_sim = {mt: [] for mt in a.metric}, {mt: [] for mt in a.metric}
    f_stage, t_sort = {mt: [] for mt in flagged}, []
    for _ in range(a.reps):
        t_search.append(search())
        # the search's answer as the stage finds it: records, term characters, bytes its gathers touch
        if not t_both:
            counts = dn.cpu().numpy().astype(np.int64)
            keys = dk.cpu().numpy().view(np.uint32).reshape(nq, stride)
            klen = np.zeros(ix.num_keys(), dtype=np.int64)
            used = np.unique(np.concatenate([keys[i, :counts[i]] for i in range(nq)]))
            for k in used:
                klen[k] = len(sim_ref.normalise(ix.key(int(k))))  # one key per row: its term is the key normalised
            lens = np.concatenate([klen[keys[i, :counts[i]]] for i in range(nq)])
            records, term_chars = int(counts.sum()), int(lens.sum())
            # key id (streamed), then three dependent random reads (key -> term, its two offsets, its bytes)
            gather_bytes = int(4 * records + 2 * SECTOR * records + (SECTOR * ((lens + 3 + SECTOR - 1) // SECTOR)).sum())
            for _ in range(a.reps):  # (the search's answer is still in place: nothing re-ranked it yet)
                t_sim.append(similarity_alone())
                for mt in a.metric:
                    m_sim[mt].append(similarity_alone(mt))
        both, stage = search_rerank()
        t_both.append(both)
        t_stage.append(stage)
        for mt in a.metric:
            m_stage[mt].append(search_rerank(mt)[1])
        for mt in flagged:
            f_stage[mt].append(search_sorted_rerank(mt))
        if a.token_sort:
            t_sort.append(sort_alone())
    kept = int(dn.cpu().numpy().astype(np.int64).sum())
    m = [len(sim_ref.normalise(q)) for q in queries]
    long_q = np.array([x > 64 for x in m])
    ms, mb, mg, mv = (statistics.median(x) for x in (t_search, t_both, t_stage, t_sim))
    token = None
    if a.token_sort:
        plain = {"levenshtein": mg, **{mt: statistics.median(m_stage[mt]) for mt in a.metric}}
        terms = {sim_ref.normalise(w) for w in words}
        ts_chars = sum(len(token_ref.sorted_term(t)) for t in terms)
        token = {"token_sort_kernel_ms": spread(t_sort), "query_bytes": int(offs[-1]),
                 "first_flagged_call_ms": round(build_ms, 3), "sorted_term_bytes": ts_chars + 8 + 8 * (len(terms) + 1),
                 "flagged": {mt: {"rerank_stage_ms": spread(f_stage[mt]),
                                  "ratio_to_unflagged": round(statistics.median(f_stage[mt]) / plain[mt], 4)}
                             for mt in flagged}}
    print(json.dumps({
        "rows": a.rows, "queries": nq, "threshold": a.threshold, "limit": a.limit, "min_similarity": a.min_similarity,
        "reps": a.reps, "warmup": a.warmup,
        "search_ms": spread(t_search), "search_rerank_ms": spread(t_both), "ratio": round(mb / ms, 4),
        "rerank_stage_ms": spread(t_stage), "similarity_kernel_ms": spread(t_sim),
        "records": records, "records_kept": kept, "term_chars": term_chars,
        "records_per_s": round(records / (mg * 1e-3)), "term_chars_per_s": round(term_chars / (mg * 1e-3)),
        "long_path_share": round(float(counts[long_q].sum()) / max(records, 1), 6),
        "terms": a.terms,
        "metrics": {mt: {"rerank_stage_ms": spread(m_stage[mt]), "similarity_kernel_ms": spread(m_sim[mt]),
                         "stage_ratio": round(statistics.median(m_stage[mt]) / mg, 4)} for mt in a.metric},
        **({"token_sort": token} if token else {}),
        "gather_bytes": gather_bytes, "gather_GBps_similarity": round(gather_bytes / (mv * 1e-3) / 1e9, 2),
        "version": _native.lib().ngsVersion().decode()}))
    ix.dispose()


if __name__ == "__main__":
    main()
