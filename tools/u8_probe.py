#!/usr/bin/env python3
"""scoreBatchU8 against scoreBatchW on the same queries, and the device decoder's own time
("UTF-8 front end").

A 200,000-row g = 2 wide library from tests/test_gpu_wide.py's wide_corpus, 4,096 queries of
6..20 characters cut from its keys, threshold 0.3, limit 100, one process. After 5 warm-ups of
each, the two calls are timed alternately (host clock around the call, which returns with the
results on the host) and the medians reported with the 10th / 90th percentiles as the spread.
The decoder (count + scan + write) is timed with HIP events around ngsUtf8Decode on a stream, and
set beside prep_kernel_ms of ngsLastStats for the same batch. Prints one JSON line.

    python tools/u8_probe.py [--rows 200000] [--queries 4096] [--reps 30]
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
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402  (one HIP runtime per process: torch's first)

import stringsearchlib_amd as ssl  # noqa: E402
from stringsearchlib_amd import _native  # noqa: E402
from test_gpu_wide import wide_corpus  # noqa: E402


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--threshold", type=float, default=0.3)
    ap.add_argument("--limit", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("u8_probe: no GPU")
    rng = random.Random(2024)
    words = wide_corpus(rng, a.rows, 1, 6, 24)
    ix = ssl.Utf8StringIndex(words, 1, None, gram_size=2)
    qs = []
    while len(qs) < a.queries:
        src = rng.choice(words).strip()
        n = rng.randint(6, 20)
        if len(src) >= n:
            o = rng.randrange(len(src) - n + 1)
            qs.append(src[o:o + n])
    L = _native.lib()
    nq = len(qs)
    q8 = (C.c_char_p * nq)(*[q.encode() for q in qs])
    U = C.POINTER(C.c_uint32)
    arrs = [(C.c_uint32 * (len(q) + 1))(*map(ord, q), 0) for q in qs]
    q32 = (U * nq)(*[C.cast(x, U) for x in arrs])
    counts = (C.c_uint32 * nq)()

    def call_u8():
        res, sc = C.POINTER(C.POINTER(C.c_char))(), C.POINTER(C.c_float)()
        t = time.perf_counter()
        n = L.scoreBatchU8(ix.handle, q8, nq, a.threshold, a.limit, counts, C.byref(res), C.byref(sc))
        dt = time.perf_counter() - t
        L.release(ix.handle, res, sc)
        return dt * 1e3, n, sum(counts)

    def call_w():
        res, sc = C.POINTER(U)(), C.POINTER(C.c_float)()
        t = time.perf_counter()
        n = L.scoreBatchW(ix.handle, q32, nq, a.threshold, a.limit, counts, C.byref(res), C.byref(sc))
        dt = time.perf_counter() - t
        L.releaseW(ix.handle, res, sc)
        return dt * 1e3, n, sum(counts)

    for _ in range(5):
        r8, rw = call_u8(), call_w()
    assert r8[1:] == rw[1:] and r8[1] > 0, (r8, rw)  # same answer sizes before any timing is trusted
    t8, tw = [], []
    for _ in range(a.reps):
        t8.append(call_u8()[0])
        tw.append(call_w()[0])

    # the decoder alone, HIP events on one stream
    enc = [q.encode() for q in qs]
    offs = [0]
    for e in enc:
        offs.append(offs[-1] + len(e))
    dev = torch.device("cuda:0")
    raw = torch.frombuffer(bytearray(b"".join(enc)), dtype=torch.uint8).to(dev)
    off = torch.tensor(offs, dtype=torch.int64, device=dev)
    out = torch.zeros(4 * offs[-1], dtype=torch.uint8, device=dev)
    out_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream()
    dec = []
    for i in range(5 + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        ssl.utf8_decode_device(raw.data_ptr(), off.data_ptr(), nq, out.data_ptr(), out.numel(), out_off.data_ptr(),
                               st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        if i >= 5:
            dec.append(e0.elapsed_time(e1))
    ix.set_timing(True)
    call_u8()
    prep = ix.last_stats()["prep_kernel_ms"]
    ix.set_timing(False)
    m8, mw = statistics.median(t8), statistics.median(tw)
    print(json.dumps({
        "rows": a.rows, "queries": nq, "threshold": a.threshold, "limit": a.limit, "reps": a.reps,
        "utf8_bytes": offs[-1], "utf32_bytes": 4 * sum(len(q) for q in qs),
        "scoreBatchU8_ms": {"median": round(m8, 4), "p10": round(pct(t8, 0.1), 4), "p90": round(pct(t8, 0.9), 4)},
        "scoreBatchW_ms": {"median": round(mw, 4), "p10": round(pct(tw, 0.1), 4), "p90": round(pct(tw, 0.9), 4)},
        "u8_over_w": round(m8 / mw, 4),
        "decoder_ms": {"median": round(statistics.median(dec), 4), "p10": round(pct(dec, 0.1), 4),
                       "p90": round(pct(dec, 0.9), 4)},
        "prep_kernel_ms": round(prep, 4), "version": L.ngsVersion().decode()}))
    ix.dispose()


if __name__ == "__main__":
    main()
