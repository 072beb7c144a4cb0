#!/usr/bin/env python3
"""What dead keys cost an index set, and the drop kernel against the compaction a caller could write
with torch.

Workload: tools/set_bench.py's (1M rows, no weights, a set of 4 equal parts, batches of 4,096 queries at
threshold 0.3 and limit 100, one process, one GPU). Times from HIP events on one stream, --reps samples
each after a warm-up of each, the routes alternating:
  ngsSetSearchDevice on sets over the same four members with 0, 0.1 %, 1 % and 10 % of the keys dead at
  random (a member in several sets has one mask per set), and with the first member wholly dead;
  ngsSetSearchDevice on a set rebuilt over the rows the 10 % plan leaves, and what that rebuild took
  (indexN of the four parts and ngsSetCreate, wall clock, once);
  ngsSearchDevice on one member alone, into a block kept between the calls, at the set's limit and at
  the limit of its first over-fetch (128 at limit 100): what the deeper search itself costs;
  k_drop_dead alone (ngsDropDeadDevice) on fabricated full rows: 4,096 rows of stride 164 cut to limit
  100, a quarter of the keys dead, and the same compaction with torch on the device (a stable sort of
  the dead flags, a gather, the cut).
A sample of a compaction is --launches calls back to back between the two events, divided by their
number, each on a copy of the block of its own (the kernel works in place): the copies are restored
outside the timing. The set with 10 % dead is compared with the rebuilt set (counts and score bits in
full, the key strings at 2,000 records), the kernel's block with the torch block. Prints one JSON line.

    python tools/set_dead_bench.py [--rows 1000000] [--reps 50] [--launches 20]
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

from bench import Corpus  # noqa: E402
from stringsearchlib_amd import _native  # noqa: E402

PARTS = 4
FRACTIONS = (("dead_0", 0.0), ("dead_0p1pct", 0.001), ("dead_1pct", 0.01), ("dead_10pct", 0.1))


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def block(B, stride, dev):
    return (torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B * stride, dtype=torch.int32, device=dev),
            torch.zeros(B * stride, dtype=torch.float32, device=dev))


def ptr(blk):
    return [t.data_ptr() for t in blk]


def rows_of(B, n, k, v):
    n, k, v = n.cpu().numpy(), k.cpu().numpy().reshape(B, -1), v.cpu().numpy().reshape(B, -1).view(np.uint32)
    live = np.arange(k.shape[1])[None, :] < n[:, None]
    return n, k[live], v[live]


def build_parts(L, addresses):
    """indexN over four equal cuts of an array of word addresses, and a set of them."""
    arr = (C.c_uint64 * len(addresses)).from_buffer_copy(np.ascontiguousarray(addresses, dtype=np.uint64).tobytes())
    base = C.addressof(arr)
    cuts = [len(addresses) * p // PARTS for p in range(PARTS + 1)]
    members = []
    for lo, hi in zip(cuts, cuts[1:]):
        h = L.indexN(C.cast(base + 8 * lo, C.POINTER(C.c_char_p)), hi - lo, 1, None)
        if not h:
            raise SystemExit("set_dead_bench: indexN of a part failed")
        members.append(h)
    return members, new_set(L, members), arr


def new_set(L, members):
    sid = L.ngsSetCreate((C.c_uint32 * PARTS)(*members), PARTS)
    if not sid:
        raise SystemExit(f"set_dead_bench: ngsSetCreate failed ({L.ngsLastError(1)})")
    return sid


def key_of(L, sid, g):
    hh, kk = C.c_uint32(), C.c_uint32()
    L.ngsSetLocate(sid, int(g), C.byref(hh), C.byref(kk))
    return C.string_at(L.ngsKey(hh.value, kk.value))


class Drop:
    """The compaction of fabricated full rows: `copies` blocks for the kernel, one pristine one."""

    def __init__(self, L, st, B, stride, limit, n_keys, copies, dev):
        g = torch.Generator(device="cpu").manual_seed(3)
        self.L, self.st, self.B, self.stride, self.limit, self.n_keys = L, st, B, stride, limit, n_keys
        gaps = torch.randint(1, n_keys // stride, (B, stride), generator=g)
        ids = (gaps.cumsum(dim=1) - 1).int()  # distinct, ascending, below n_keys
        scores = (100.0 - (torch.arange(stride) * 8 // stride).float() * 7.5).repeat(B)
        self.pristine = (torch.full((B,), stride, dtype=torch.int32, device=dev), ids.reshape(-1).to(dev), scores.to(dev))
        dead = torch.rand(n_keys, generator=g) < 0.25
        bits = np.packbits(np.pad(dead.numpy(), (0, -n_keys % 32)), bitorder="little").view(np.uint32)
        self.mask = torch.from_numpy(bits.view(np.int32).copy()).to(dev)
        self.dead = dead.to(dev)
        self.copies = [tuple(t.clone() for t in self.pristine) for _ in range(copies)]
        self.short = torch.zeros(1, dtype=torch.int32, device=dev)
        self.at = 0
        self.torch_block = None

    def restore(self):
        for c in self.copies:
            for dst, src in zip(c, self.pristine):
                dst.copy_(src)
        self.at = 0

    def kernel(self):
        blk = self.copies[self.at % len(self.copies)]
        self.at += 1
        return self.L.ngsDropDeadDevice(*ptr(blk), self.B, self.stride, self.mask.data_ptr(), self.n_keys, self.limit,
                                        self.short.data_ptr(), self.st.cuda_stream)

    def torch(self):
        n, k, v = self.pristine
        with torch.cuda.stream(self.st):
            keys = k.view(self.B, self.stride)
            gone = self.dead[keys.long()]
            o = torch.sort(gone.to(torch.uint8), dim=1, stable=True).indices[:, :self.limit]  # the live records first, in order
            self.torch_block = ((~gone).sum(1).clamp(max=self.limit).int(), keys.gather(1, o),
                                v.view(self.B, self.stride).gather(1, o))
        return 0

    def blocks_equal(self):
        n, k, v = self.copies[0]
        a = rows_of(self.B, n, k, v)
        b = rows_of(self.B, *(t.contiguous().view(-1) if i else t for i, t in enumerate(self.torch_block)))
        return bool(all(np.array_equal(x, y) for x, y in zip(a, b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--threshold", type=float, default=0.3)
    ap.add_argument("--limit", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("set_dead_bench: no GPU")
    L = _native.lib()
    corpus = Corpus(a.rows)
    addresses = np.ctypeslib.as_array(C.cast(corpus.words, C.POINTER(C.c_uint64)), shape=(a.rows,)).copy()
    members, first_set, keep0 = build_parts(L, addresses)
    total = L.ngsSetNumKeys(first_set)
    rng = np.random.default_rng(7)
    sets, dead_ids = {}, {}
    for name, frac in FRACTIONS:
        sid = first_set if name == "dead_0" else new_set(L, members)
        ids = np.sort(rng.choice(total, int(total * frac), replace=False)).astype(np.uint32)
        if len(ids) and L.ngsSetRemove(sid, ids.ctypes.data_as(C.POINTER(C.c_uint32)), len(ids)) != len(ids):
            raise SystemExit("set_dead_bench: ngsSetRemove failed")
        sets[name], dead_ids[name] = sid, ids
    sid = new_set(L, members)
    ids = np.arange(L.ngsNumKeys(members[0]), dtype=np.uint32)
    if L.ngsSetRemove(sid, ids.ctypes.data_as(C.POINTER(C.c_uint32)), len(ids)) != len(ids):
        raise SystemExit("set_dead_bench: ngsSetRemove failed")
    sets["member_dead"] = sid

    # the set rebuilt over the rows the 10 % plan leaves: what a caller without ngsSetRemove does
    gone = {key_of(L, first_set, g) for g in dead_ids["dead_10pct"]}
    words = [C.string_at(int(p)) for p in addresses]
    live = np.array([w not in gone for w in words])
    t0 = time.perf_counter()
    re_members, re_set, keep1 = build_parts(L, addresses[live])
    rebuild_s = time.perf_counter() - t0
    sets["rebuilt_10pct"] = re_set

    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    s = st.cuda_stream
    B, lim, thr = a.queries, a.limit, a.threshold
    raw, offs = corpus.queries(B)
    d_raw = torch.from_numpy(np.frombuffer(raw + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    out = {k: block(B, lim, dev) for k in sets}

    def search(name):
        return lambda: L.ngsSetSearchDevice(sets[name], d_raw.data_ptr(), d_off.data_ptr(), B, thr, lim, lim,
                                            *ptr(out[name]), s)

    n = a.launches
    drop = Drop(L, st, B, 164, 100, 400_000, n, dev)
    torch.cuda.synchronize()

    def timed(fn, calls=1, before=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before:
            before()
        torch.cuda.synchronize()
        e0.record(st)
        for _ in range(calls):
            if fn():
                raise SystemExit("set_dead_bench: a call failed")
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1) / calls

    routes = {f"{k}_ms": (search(k), 1, None) for k in sets}
    # where a dead key's cost lies: one member searched alone into a block kept between the calls, at the
    # set's limit and at the limit its first over-fetch asks for
    fetch = 128 if lim <= 112 else lim + max(lim, 64)  # ngs_set.h: dead_first_fetch
    one = {L_: block(B, L_, dev) for L_ in (lim, fetch)}
    for L_ in (lim, fetch):
        routes[f"member_search_limit_{L_}_ms"] = (
            (lambda L_=L_: L.ngsSearchDevice(members[1], d_raw.data_ptr(), d_off.data_ptr(), B, thr, L_, L_, *ptr(one[L_]), s)),
            1, None)
    routes["drop_kernel_ms"] = (drop.kernel, n, drop.restore)
    routes["drop_torch_ms"] = (drop.torch, n, None)
    for fn, calls, before in routes.values():  # warm-up of each
        for _ in range(3):
            timed(fn, calls, before)
    times = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, (fn, calls, before) in routes.items():
            times[k].append(timed(fn, calls, before))

    # the set with 10 % dead against the rebuilt one: counts and score bits in full, strings at 2,000 records
    r_dead, r_new = rows_of(B, *out["dead_10pct"]), rows_of(B, *out["rebuilt_10pct"])
    same_scores = bool(np.array_equal(r_dead[0], r_new[0]) and np.array_equal(r_dead[2], r_new[2]))
    same_keys = same_scores
    probe = np.random.default_rng(1).integers(0, max(1, len(r_dead[1])), min(2000, len(r_dead[1])))
    for j in probe.tolist() if same_scores else []:
        same_keys &= key_of(L, sets["dead_10pct"], r_dead[1][j]) == key_of(L, re_set, r_new[1][j])
    dead_hits = int(np.isin(r_dead[1], dead_ids["dead_10pct"]).sum())
    stats = {}
    for k, sid in sets.items():
        v = (C.c_uint64 * 3)()
        L.ngsSetDeadStats(sid, v, 3)
        stats[k] = {"drop_launches": v[0], "re_searches": v[1], "max_over_fetch": v[2]}
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "rows": a.rows, "parts": PARTS, "queries": B, "threshold": thr, "limit": lim, "reps": a.reps,
        "launches_per_drop_sample": n, "set_keys": total, "records_no_dead": int(rows_of(B, *out["dead_0"])[0].sum()),
        "records_10pct_dead": int(r_dead[0].sum()),
        **{k: spread(v) for k, v in times.items()},
        "rebuild_s": round(rebuild_s, 3),
        "dead_10pct_over_no_dead": round(med["dead_10pct_ms"] / med["dead_0_ms"], 4),
        "drop_rows": {"rows": B, "stride": 164, "limit": 100, "dead_fraction": 0.25},
        "drop_kernel_over_torch": round(med["drop_kernel_ms"] / med["drop_torch_ms"], 4),
        "drop_blocks_equal": drop.blocks_equal(), "dead_hits_returned": dead_hits,
        "counts_and_scores_equal_rebuilt_set": same_scores, "probed_key_strings_equal_rebuilt_set": bool(same_keys),
        "dead_stats": stats, "version": L.ngsVersion().decode()}))
    for sid in sets.values():
        L.ngsSetDispose(sid)
    for h in members + re_members:
        L.dispose(h)
    del keep0, keep1


if __name__ == "__main__":
    main()
