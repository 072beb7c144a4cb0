#!/usr/bin/env python3
"""An index set against one index, and the merge kernel against the merge a caller could write with
torch.

Workload: tools/join_bench.py's library (1M rows, no weights), batches of 4,096 queries at threshold
0.3 and limit 100, one process, one GPU. Times from HIP events on one stream, --reps samples each after
a warm-up of each, the routes alternating:
  (a) one index over all rows, ngsSearchDevice;
  (b) a set of 4 equal parts, ngsSetSearchDevice; and k_merge_parts' own time, ngsMergeResultsDevice over
      the four members' blocks (searched once, outside the timing);
  (c) the merge on the same four blocks with torch on the device: the blocks concatenated with a
      gathered length column, stable-sorted by id, then length, then score, and cut to the limit.
A sample of a merge is --launches calls back to back between the two events, divided by their number:
one launch of some ten microseconds would measure the events as much as the kernel.
The workload's rows are nearly empty, so the two merges are also timed on fabricated full rows in merge
order (scores in 8 steps down a row, ids ascending, lengths ascending with the id): 4 parts of
stride 100 at limit 100 for 4,096 queries (400 records a query, the LDS path), and 4 parts of stride
3,000 at limit 0 for 256 queries (12,000 records a query out, the HBM path).
The kernel's block, the torch block and (a)'s block are compared at full size. Prints one JSON line.

    python tools/set_bench.py [--rows 1000000] [--reps 50] [--launches 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime per process: torch's first)

from bench import Corpus, build_index  # noqa: E402
from stringsearchlib_amd import _native  # noqa: E402

PARTS = 4
LIMIT_ALL = 2**31 - 1


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def block(B, stride, dev):
    return (torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B * stride, dtype=torch.int32, device=dev),
            torch.zeros(B * stride, dtype=torch.float32, device=dev))


def ptr(blk):
    return [t.data_ptr() for t in blk]


def rows_of(B, n, k, v):
    """A block's live records, flat: (counts, key ids, score bits)."""
    n, k, v = n.cpu().numpy(), k.cpu().numpy().reshape(B, -1), v.cpu().numpy().reshape(B, -1).view(np.uint32)
    live = np.arange(k.shape[1])[None, :] < n[:, None]
    return n, k[live], v[live]


def same(x, y):
    return bool(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]))


class Merge:
    """One merge of PARTS blocks of one stride for B queries: by the kernel and by torch, on stream st."""

    def __init__(self, L, st, blocks, lens, nk, base, B, stride, limit):
        self.L, self.st, self.blocks, self.lens, self.nk, self.base = L, st, blocks, lens, nk, base
        self.B, self.stride, self.limit = B, stride, limit
        self.out = min(limit or LIMIT_ALL, PARTS * stride)
        dev = blocks[0][0].device
        self.kernel_block = block(B, self.out, dev)
        self.desc = (_native.MergePart * PARTS)()
        for p, d in enumerate(self.desc):
            d.dCounts, d.dKeys, d.dScores = ptr(blocks[p])
            d.stride, d.keyBase, d.dKeyLen, d.nKeys = stride, base[p], lens[p].data_ptr(), nk[p]
        self.col = torch.arange(stride, device=dev)[None, :]
        self.torch_block = None

    def kernel(self):
        return self.L.ngsMergeResultsDevice(self.desc, PARTS, self.B, self.limit, self.out, *ptr(self.kernel_block),
                                            self.st.cuda_stream)

    def torch(self):
        """The same merge with torch: concatenate, three stable sorts (id, length, score), cut."""
        B, stride = self.B, self.stride
        with torch.cuda.stream(self.st):
            live = torch.cat([self.col < c[:, None] for c, _, _ in self.blocks], dim=1)
            local = [k.view(B, stride).long() for _, k, _ in self.blocks]
            gid = torch.cat([k + self.base[p] for p, k in enumerate(local)], dim=1)
            ln = torch.cat([self.lens[p][k.clamp(0, self.nk[p] - 1)] for p, k in enumerate(local)], dim=1)
            sc = torch.cat([v.view(B, stride) for _, _, v in self.blocks], dim=1)
            sc = torch.where(live, sc, torch.full_like(sc, float("-inf")))  # dead cells last
            o = torch.sort(gid, dim=1, stable=True).indices
            o = o.gather(1, torch.sort(ln.gather(1, o), dim=1, stable=True).indices)
            o = o.gather(1, torch.sort(sc.gather(1, o), dim=1, stable=True, descending=True).indices)[:, :self.out]
            self.torch_block = (live.sum(1).clamp(max=self.out).int(), gid.gather(1, o).int(), sc.gather(1, o))
        return 0

    def blocks_equal(self):
        return same(rows_of(self.B, *self.kernel_block), rows_of(self.B, *self.torch_block))


def full_rows(B, stride, n_keys, dev, seed):
    """PARTS fabricated blocks of full rows in merge order and their length tables."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    blocks, lens = [], []
    steps = (100.0 - (torch.arange(stride) * 8 // stride).float() * 7.5)  # 8 score classes down a row
    for _ in range(PARTS):
        gaps = torch.randint(1, n_keys // stride, (B, stride), generator=g)
        ids = gaps.cumsum(dim=1) - 1  # distinct, ascending, below n_keys
        blocks.append((torch.full((B,), stride, dtype=torch.int32, device=dev),
                       ids.int().reshape(-1).to(dev), steps.repeat(B).to(dev)))
        lens.append((3 + torch.arange(n_keys) // 64).int().to(dev))
    return blocks, lens


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
        raise SystemExit("set_bench: no GPU")
    L = _native.lib()
    corpus = Corpus(a.rows)
    whole = build_index(corpus, False, 0)
    cuts = [a.rows * p // PARTS for p in range(PARTS + 1)]
    words = C.cast(corpus.words, C.c_void_p).value
    members = []
    for lo, hi in zip(cuts, cuts[1:]):
        h = L.indexN(C.cast(words + 8 * lo, C.POINTER(C.c_char_p)), hi - lo, 1, None)
        if not h:
            raise SystemExit("set_bench: indexN of a part failed")
        members.append(h)
    sid = L.ngsSetCreate((C.c_uint32 * PARTS)(*members), PARTS)
    if not sid:
        raise SystemExit(f"set_bench: ngsSetCreate failed ({L.ngsLastError(1)})")
    nk = [L.ngsNumKeys(h) for h in members]
    base = [sum(nk[:p]) for p in range(PARTS)]

    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    s = st.cuda_stream
    B, lim, thr = a.queries, a.limit, a.threshold
    raw, offs = corpus.queries(B)
    d_raw = torch.from_numpy(np.frombuffer(raw + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_off = torch.tensor(offs, dtype=torch.int64, device=dev)

    one, merged = block(B, lim, dev), block(B, lim, dev)
    search_one = lambda: L.ngsSearchDevice(whole, d_raw.data_ptr(), d_off.data_ptr(), B, thr, lim, lim, *ptr(one), s)
    search_set = lambda: L.ngsSetSearchDevice(sid, d_raw.data_ptr(), d_off.data_ptr(), B, thr, lim, lim, *ptr(merged), s)

    # the members' blocks and length tables, as a caller of ngsMergeResultsDevice holds them
    blocks = [block(B, lim, dev) for _ in range(PARTS)]
    lens = [torch.zeros(n, dtype=torch.int32, device=dev) for n in nk]
    for p in range(PARTS):
        if L.ngsSearchDevice(members[p], d_raw.data_ptr(), d_off.data_ptr(), B, thr, lim, lim, *ptr(blocks[p]), s) or \
                L.ngsKeyLengthsDevice(members[p], 0, nk[p], lens[p].data_ptr(), s):
            raise SystemExit("set_bench: a member's search failed")
    st.synchronize()
    work = Merge(L, st, blocks, lens, nk, base, B, lim, lim)
    fab = 100_000  # keys per fabricated part
    fab_base = [fab * p for p in range(PARTS)]
    lds = Merge(L, st, *full_rows(B, 100, fab, dev, 1), [fab] * PARTS, fab_base, B, 100, 100)
    hbm = Merge(L, st, *full_rows(256, 3000, fab, dev, 2), [fab] * PARTS, fab_base, 256, 3000, 0)
    torch.cuda.synchronize()

    def timed(fn, calls=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        for _ in range(calls):
            if fn():
                raise SystemExit("set_bench: a call failed")
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1) / calls

    n = a.launches
    routes = {"one_index_ms": (search_one, 1), "set_ms": (search_set, 1),
              "merge_kernel_ms": (work.kernel, n), "merge_torch_ms": (work.torch, n),
              "full_rows_kernel_ms": (lds.kernel, n), "full_rows_torch_ms": (lds.torch, n),
              "hbm_rows_kernel_ms": (hbm.kernel, n), "hbm_rows_torch_ms": (hbm.torch, n)}
    for fn, calls in routes.values():  # warm-up of each
        for _ in range(3):
            timed(fn, calls)
    times = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, (fn, calls) in routes.items():
            times[k].append(timed(fn, calls))

    r_set = rows_of(B, *merged)
    # (a)'s ids are the whole index's and the set's are global ids: counts and score bits are compared
    # in full, the key strings at 2,000 records drawn at random
    n_one, k_one, v_one = rows_of(B, *one)
    same_scores = bool(np.array_equal(n_one, r_set[0]) and np.array_equal(v_one, r_set[2]))
    probe = np.random.default_rng(1).integers(0, max(1, len(k_one)), min(2000, len(k_one)))
    hh, kk = C.c_uint32(), C.c_uint32()
    same_keys = same_scores
    for j in probe.tolist() if same_scores else []:
        L.ngsSetLocate(sid, int(r_set[1][j]), C.byref(hh), C.byref(kk))
        same_keys &= C.string_at(L.ngsKey(whole, int(k_one[j]))) == C.string_at(L.ngsKey(hh.value, kk.value))
    med = {k: statistics.median(v) for k, v in times.items()}
    ratio = lambda x, y: round(med[x] / med[y], 4)
    print(json.dumps({
        "rows": a.rows, "parts": PARTS, "queries": B, "threshold": thr, "limit": lim, "reps": a.reps,
        "launches_per_merge_sample": n,
        "keys": L.ngsNumKeys(whole), "set_keys": L.ngsSetNumKeys(sid), "records": int(r_set[0].sum()),
        **{k: spread(v) for k, v in times.items()},
        "set_over_one_index": ratio("set_ms", "one_index_ms"),
        "merge_kernel_over_torch": ratio("merge_kernel_ms", "merge_torch_ms"),
        "full_rows": {"queries": lds.B, "stride": lds.stride, "limit": lds.limit, "records_in_per_query": 400},
        "full_rows_kernel_over_torch": ratio("full_rows_kernel_ms", "full_rows_torch_ms"),
        "hbm_rows": {"queries": hbm.B, "stride": hbm.stride, "limit": hbm.limit, "records_in_per_query": 12000},
        "hbm_rows_kernel_over_torch": ratio("hbm_rows_kernel_ms", "hbm_rows_torch_ms"),
        "kernel_block_equals_set_block": same(rows_of(B, *work.kernel_block), r_set),
        "torch_block_equals_kernel_block": work.blocks_equal(),
        "full_rows_blocks_equal": lds.blocks_equal(), "hbm_rows_blocks_equal": hbm.blocks_equal(),
        "set_counts_and_scores_equal_one_index": same_scores, "probed_key_strings_equal_one_index": bool(same_keys),
        "version": L.ngsVersion().decode()}))
    L.ngsSetDispose(sid)
    for h in members + [whole]:
        L.dispose(h)


if __name__ == "__main__":
    main()
