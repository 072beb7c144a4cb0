"""Multi-rank path of bench.py / shard.py on CPU: world size 2 over gloo.

Each rank takes its contiguous query slice (shard_bounds) and scores it, with the CPU oracle
standing in for the GPU searcher, since this container has no GPU. It writes the fixed-stride
device layout that ngsSearchDevice produces, compacts it and gathers it to rank 0. Rank 0
checks that the gathered per-rank results, concatenated, equal the whole batch scored in
one piece.
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle_py import OracleIndex
from stringsearchlib_amd import shard, synth

LIMIT = 20
THR = 0.25


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _device_layout(oi, queries, stride):
    """(counts[B], keys[B*stride], scores[B*stride]) as ngsSearchDevice writes them."""
    B = len(queries)
    counts = torch.zeros(B, dtype=torch.int32)
    keys = torch.full((B * stride,), -1, dtype=torch.int32)
    scores = torch.full((B * stride,), -1.0, dtype=torch.float32)
    for i, q in enumerate(queries):
        ids, sc = oi.score_ids(q, THR, LIMIT)
        counts[i] = len(ids)
        keys[i * stride:i * stride + len(ids)] = torch.tensor(ids, dtype=torch.int32)
        scores[i * stride:i * stride + len(sc)] = torch.tensor(sc, dtype=torch.float32)
    return counts, keys, scores


def _worker(rank, world, port, result_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        words, wts, rng = synth.gen_corpus(3000, seed=7)
        queries = synth.gen_queries(words, 1, 65, rng)  # ragged: 33 + 32
        oi = OracleIndex(words, 1, wts)
        lo, hi = shard.shard_bounds(rank, world, len(queries))
        stride = LIMIT
        pad_b = shard.max_shard(world, len(queries))
        c, k, s = _device_layout(oi, queries[lo:hi], stride)
        got = shard.gather_to_root(c, k, s, stride, pad_b=pad_b)
        # without pad_b the ranks agree on the largest slice themselves (ragged 33 + 32 here)
        got_default = shard.gather_to_root(c, k, s, stride)
        if rank == 0:
            assert all(torch.equal(a, b) for x, y in zip(got, got_default) for a, b in zip(x, y))
        # the in-flight form bench.py uses: results written into a GatherBuffer's views (as
        # ngsSearchDevice does), gathered without any size exchange, decoded after wait()
        gb = shard.GatherBuffer(hi - lo, stride, pad_b)
        gb.counts.copy_(c)
        gb.keys.copy_(k)
        gb.scores.copy_(s)
        got_async = shard.gather_to_root(gb, async_op=True).wait()
        if rank == 0:
            assert all(torch.equal(a, b) for x, y in zip(got, got_async) for a, b in zip(x, y))
        else:
            assert got is None and got_async is None
        # the packed form bench.py's step loop uses: records packed (pack_torch stands in for
        # ngsPackResults), the ranks agree on the largest total, the gather moves only that prefix
        pg = shard.PackedGather(hi - lo, stride, pad_b)
        pg.counts.copy_(c)
        pg.keys.copy_(k)
        pg.scores.copy_(s)
        pend = shard.gather_packed(pg.pack(), async_op=True)
        assert pend.words < 1 + pad_b * (1 + 2 * stride)  # fewer words than the fixed layout
        got_packed = pend.wait()
        if rank == 0:
            assert all(torch.equal(a, b) for x, y in zip(got, got_packed) for a, b in zip(x, y))
        else:
            assert got_packed is None
        if rank == 0:
            flat = []
            for counts, keys, scores in got:
                o = 0
                for n in counts.tolist():
                    flat.append((keys[o:o + n].tolist(), scores[o:o + n].tolist()))
                    o += n
            want = [tuple(map(list, oi.score_ids(q, THR, LIMIT))) for q in queries]
            ok = len(flat) == len(want) and all(
                a == list(b[0]) and torch.equal(torch.tensor(sa, dtype=torch.float32),
                                                 torch.tensor(b[1], dtype=torch.float32))
                for (a, sa), b in zip(flat, want))
            with open(result_path, "w") as f:
                f.write("ok" if ok else f"mismatch: {flat[:2]} vs {want[:2]}")
        oi.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_gather_matches_single_batch(tmp_path):
    out = tmp_path / "result.txt"
    mp.spawn(_worker, args=(2, _free_port(), str(out)), nprocs=2, join=True)
    assert out.read_text() == "ok"


def test_gather_buffer_layout():
    gb = shard.GatherBuffer(3, 4, pad_b=5)
    gb.counts.copy_(torch.tensor([2, 0, 4], dtype=torch.int32))
    gb.keys.copy_(torch.arange(12, dtype=torch.int32))
    gb.scores.copy_(torch.arange(12, dtype=torch.float32) / 2)
    c, k, s = shard.GatherBuffer.decode(gb.buf, 4, 5)
    assert c.tolist() == [2, 0, 4] and k.tolist() == [0, 1, 8, 9, 10, 11]
    assert s.tolist() == [0.0, 0.5, 4.0, 4.5, 5.0, 5.5]
    assert shard.max_shard(8, 65541) == 8193 and shard.max_shard(2, 64) == 32


def test_shard_bounds_cover_batch():
    for world in (1, 2, 3, 8):
        spans = [shard.shard_bounds(r, world, 65536 + 5) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == 65541
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_pack_torch_reads_a_count_above_the_stride_as_the_stride():
    """The CPU stand-in of ngsPackResults defines a count above the stride as the library does:
    the prefix sum and the copy both read it as the stride (a negative int32 is a large uint32), so
    the total is the number of records written, no record sits behind a hole, and decode accepts
    the buffer with the clamped counts' sum."""
    n, stride = 7, 4
    raw = [2, stride + 1, 0, -2**31, 3, -1, stride]  # 2^31 and 0xFFFFFFFF as int32
    clamped = [2, 4, 0, 4, 3, 4, 4]
    pg = shard.PackedGather(n, stride, pad_b=9)
    pg.counts.copy_(torch.tensor(raw, dtype=torch.int32))
    pg.keys.copy_(torch.arange(100, 100 + n * stride, dtype=torch.int32))
    pg.scores.copy_(torch.arange(n * stride, dtype=torch.float32) / 4)
    pg.records.fill_(-7)
    pg.pack()
    total = sum(clamped)
    assert pg.offsets.tolist() == [0, 2, 6, 6, 10, 13, 17, 21] and int(pg.buf[1]) == total
    want_k = [100 + q * stride + i for q in range(n) for i in range(clamped[q])]
    rec = pg.records[:2 * total].view(total, 2)
    assert rec[:, 0].tolist() == want_k
    assert rec[:, 1].contiguous().view(torch.float32).tolist() == [(k - 100) / 4 for k in want_k]
    assert bool((pg.records[2 * total:] == -7).all())  # nothing written past the total
    # the buffer still holds the block's counts as written: decode, told the stride, reads them as
    # the packer did and accepts the buffer; without the stride their sum is not the total
    assert pg.counts.tolist() == raw
    c, k, s = shard.PackedGather.decode(pg.buf, 9, stride)
    assert c.tolist() == clamped and k.tolist() == want_k
    assert s.tolist() == [(x - 100) / 4 for x in want_k]
    with pytest.raises(ValueError):
        shard.PackedGather.decode(pg.buf, 9)
    # ordinary counts decode alike with and without it
    pg.counts.copy_(torch.tensor(clamped, dtype=torch.int32))
    for got in (shard.PackedGather.decode(pg.pack().buf, 9), shard.PackedGather.decode(pg.buf, 9, stride)):
        assert got[0].tolist() == clamped and got[1].tolist() == want_k
