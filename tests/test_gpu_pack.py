"""ngsPackResults (a hipcub inclusive scan of the counts behind dOffsets[0] = 0, then k_pack_pairs,
one wave per query) against a few lines of numpy, on fabricated result blocks.

The reference is written here and is not shard.pack_torch (the CPU stand-in, tested in
test_shard.py): counts clamped to the stride, their exclusive prefix sum, and the records in query
order as {key, score bits}. Everything is compared as uint32 words: offsets, records, the untouched
tail of the record array, guard words behind both outputs, and the inputs.
"""
import numpy as np
import pytest
import torch

from oracle_py import OracleIndex

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native, shard

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PAT = 0x5EED5EED       # fills both outputs and their guard words before a call
GUARD_WORDS = 64
# score bits that a float copy could change: -0.0, subnormals, infinities, quiet and signalling NaNs
SPECIAL = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFA5A5A5, 0x7F800001,
                    0x00000000, 0x3F800000], dtype=np.uint32)


def ref_pack(counts, keys, bits, n, stride):
    """(offsets[n + 1], records[2 * total]) as uint32: a count above the stride is the stride."""
    c = np.minimum(counts.astype(np.uint64), np.uint64(stride)).astype(np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(c, out=off[1:])
    assert int(off[n]) <= 0xFFFFFFFF
    take = np.arange(stride, dtype=np.int64)[None, :] < c[:, None]
    rec = np.stack([keys.reshape(n, stride)[take], bits.reshape(n, stride)[take]], axis=1).reshape(-1)
    return off.astype(np.uint32), rec.astype(np.uint32)


def _dev(a):
    """A uint32 numpy array as an int32 tensor on the device (the bits as they are)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def _host(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


class Block:
    """A fabricated result block in ngsSearchDevice's layout and the two output arrays, each with
    guard words behind it, all filled with a pattern."""

    def __init__(self, counts, keys, bits, n, stride):
        self.n, self.stride = n, stride
        self.h = (counts.copy(), keys.copy(), bits.copy())
        self.counts = _dev(counts if n else np.zeros(1, dtype=np.uint32))
        self.keys = _dev(keys) if n else None
        self.scores = _dev(bits).view(torch.float32) if n else None
        self.off = torch.full((n + 1 + GUARD_WORDS,), PAT, dtype=torch.int32, device=DEV)
        self.rec = torch.full((2 * n * stride + GUARD_WORDS,), PAT, dtype=torch.int32, device=DEV)

    def pack(self, stream=None, null_records=False):
        stream = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return _native.lib().ngsPackResults(ptr(self.counts), ptr(self.keys), ptr(self.scores), self.n, self.stride,
                                            ptr(self.off), None if null_records else ptr(self.rec), stream or None)

    def check(self, where):
        n, stride = self.n, self.stride
        counts, keys, bits = self.h
        want_off, want_rec = ref_pack(counts, keys, bits, n, stride)
        off, rec = _host(self.off), _host(self.rec)
        total = int(want_off[n])
        bad = np.flatnonzero(off[:n + 1] != want_off)
        assert not len(bad), f"{where}: offsets differ first at {bad[0]}: {off[bad[0]]} vs {want_off[bad[0]]}"
        bad = np.flatnonzero(rec[:2 * total] != want_rec)
        assert not len(bad), f"{where}: record words differ first at {bad[0]} of {2 * total}"
        assert bool((rec[2 * total:] == PAT).all()), f"{where}: record words past 2 x {total} were written"
        assert bool((off[n + 1:] == PAT).all()), f"{where}: words behind dOffsets[n] were written"
        if n:  # the inputs are read only
            assert np.array_equal(_host(self.counts), counts) and np.array_equal(_host(self.keys), keys)
            assert np.array_equal(_host(self.scores), bits), where


PATTERNS = ["zero", "full", "random", "last", "first", "alternate"]


def make_counts(pattern, n, stride, rng):
    c = np.zeros(n, dtype=np.uint32)
    if pattern == "full":
        c[:] = stride
    elif pattern == "random":
        c[:] = rng.integers(0, stride + 1, n)
    elif pattern == "last" and n:
        c[-1] = rng.integers(1, stride + 1)
    elif pattern == "first" and n:
        c[0] = rng.integers(1, stride + 1)
    elif pattern == "alternate":
        c[1::2] = stride
    return c


def make_values(n, stride, rng):
    """Random key ids and score bits with 0, 0xFFFFFFFF and the special score bits sown in, the
    first cells of the rows included (those are copied whenever a count is not 0)."""
    m = min(n * stride, 1_000_003)  # (a large block repeats a million random words: quicker to make)
    keys = np.resize(rng.integers(0, 1 << 32, m, dtype=np.uint32), n * stride)
    bits = np.resize(rng.integers(0, 1 << 32, m, dtype=np.uint32), n * stride)
    keys[0::6] = 0
    keys[3::6] = 0xFFFFFFFF
    bits[::3] = np.resize(SPECIAL, len(bits[::3]))
    k2, b2 = keys.reshape(n, stride), bits.reshape(n, stride)
    k2[0::2, 0] = 0xFFFFFFFF
    k2[1::2, 0] = 0
    b2[:, 0] = np.resize(SPECIAL, n)
    return keys, bits


def run_patterns(n, stride, seed):
    rng = np.random.default_rng(seed)
    keys, bits = make_values(n, stride, rng)
    for pattern in PATTERNS:
        b = Block(make_counts(pattern, n, stride, rng), keys, bits, n, stride)
        assert b.pack() == 0
        b.check(f"n={n} stride={stride} {pattern}")


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 70001])
def test_batch_sizes(n):
    """Around k_pack_pairs' four queries per block and the scan's tile; 70,001 queries (stride 4)
    run past any single scan tile and through 17,501 blocks of the second kernel."""
    run_patterns(n, 4 if n > 5000 else 9, 100 + n)


@pytest.mark.parametrize("stride", [1, 63, 64, 65, 100, 130])
def test_strides_around_the_wave_loop(stride):
    """k_pack_pairs copies a query's records 64 at a time: strides of one pass, one short of it,
    one past it, and two and three passes."""
    for n in (1, 3, 5, 65, 257):
        run_patterns(n, stride, 1000 * stride + n)


def test_empty_batch_with_null_arrays():
    """n = 0 with NULL keys, scores and records: 0, dOffsets[0] = 0 and nothing else."""
    e = np.zeros(0, dtype=np.uint32)
    for stride in (0, 16):
        b = Block(e, e, e, 0, stride)
        b.counts.fill_(77)  # (must be non-NULL; nothing of it is read)
        assert b.pack(null_records=True) == 0
        off = _host(b.off)
        assert off[0] == 0 and bool((off[1:] == PAT).all())
        assert bool((_host(b.rec) == PAT).all()) and int(b.counts[0]) == 77


def _random_block(n, stride, seed):
    rng = np.random.default_rng(seed)
    keys, bits = make_values(n, stride, rng)
    return Block(make_counts("random", n, stride, rng), keys, bits, n, stride)


# The scan's scratch (pack_pairs_temp_bytes: hipcub's size query) is one 8-byte tile state per 4,096
# counts and 524 bytes: 1,108 bytes at n = 300,000, 64,972 at 33,000,000, 131,380 at 67,000,000 on
# an MI355X. The first allocation is 64 KiB, so the grow-and-replace branch needs
# n > (65,536 - 524) / 8 x 4,096 = 33.3 million: 34,000,000 asks for 66.9 KB.
N_GROW = 34_000_000


def test_scratch_buffer_grows_and_streams_keep_their_own():
    """The scan's scratch is one grow-only buffer per (device, stream), 64 KiB at first: a small
    call, one whose scan needs more (the buffer is replaced behind the stream's earlier work) and a
    small one again on one new stream; then two streams with different n, queued with no host wait
    between them. (The large call is 34 million queries at stride 1: the smallest round number
    whose scan outgrows 64 KiB; about 1 GB on the device and a few seconds.)"""
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    blocks = [_random_block(5, 7, 1), _random_block(N_GROW, 1, 2), _random_block(5, 7, 3)]
    s1.wait_stream(torch.cuda.current_stream(DEV))
    s2.wait_stream(torch.cuda.current_stream(DEV))
    for b in blocks:
        assert b.pack(s1.cuda_stream) == 0
    s1.synchronize()
    for i, b in enumerate(blocks):
        b.check(f"scratch call {i} (n={b.n})")
    pairs = [(_random_block(1000, 8, 4), s1), (_random_block(3001, 3, 5), s2), (_random_block(70001, 2, 6), s1),
             (_random_block(17, 65, 7), s2)]
    torch.cuda.synchronize(DEV)
    for b, s in pairs:
        assert b.pack(s.cuda_stream) == 0
    s1.synchronize()
    s2.synchronize()
    for i, (b, _) in enumerate(pairs):
        b.check(f"two streams call {i} (n={b.n})")


def test_counts_above_the_stride_are_read_as_the_stride():
    """A count above the stride is read as the stride by the scan as by the copy: dOffsets[n] is
    the number of records written and no query's records sit behind a hole. First a block whose
    unclamped sum would still fit the record array (three counts of stride + 1 among small ones),
    so that a library that summed the raw counts fails here without writing past anything; then
    counts of 2^31 and 0xFFFFFFFF among ordinary ones."""
    n, stride = 64, 8
    rng = np.random.default_rng(11)
    keys, bits = make_values(n, stride, rng)
    mild = rng.integers(0, 5, n).astype(np.uint32)
    mild[[5, 20, 41]] = stride + 1
    assert int(mild.sum()) <= n * stride
    b = Block(mild, keys, bits, n, stride)
    assert b.pack() == 0
    b.check("counts of stride + 1")
    wild = make_counts("random", n, stride, rng)
    wild[[0, 9, 33, 63]] = [0xFFFFFFFF, stride + 1, 1 << 31, 0xFFFFFFFF]
    wild[[10, 34]] = [0, stride]
    b = Block(wild, keys, bits, n, stride)
    assert b.pack() == 0
    b.check("counts of 2^31 and 0xFFFFFFFF")
    n, stride = 1025, 3
    keys, bits = make_values(n, stride, rng)
    every = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    every[::7] = 1 << 31
    b = Block(every, keys, bits, n, stride)
    assert b.pack() == 0
    b.check("every count above the stride")


def test_search_then_pack_end_to_end():
    """ngsSearchDevice at limit 16 into a PackedGather's views, ngsPackResults behind it on the same
    stream, decoded and compared with scoreBatch: at threshold 0.3 and at 0 (full counts), over
    two buffers used in turn as the benchmark's step loop uses them."""
    words, wts, rng = ssl.synth.gen_corpus(3000, seed=17)
    gi = ssl.StringIndex(words, 1, wts)
    oi = OracleIndex(words, 1, wts)
    limit = 16
    batches = [[w[:2] for w in words[:40]] + ssl.synth.gen_queries(words, 1, 300, rng) + [b"AB", b"", b"*", b"Q9X#"],
               [w[:2] for w in words[40:80]] + ssl.synth.gen_queries(words, 1, 257, rng) + [words[3], b"E"]]
    side = torch.cuda.Stream(DEV)
    pgs = [shard.PackedGather(max(map(len, batches)), limit, device=DEV) for _ in range(2)]
    side.wait_stream(torch.cuda.current_stream(DEV))
    packer = _native.lib().ngsPackResults
    step = 0
    with torch.cuda.stream(side):
        for qs in batches:
            raw = torch.frombuffer(bytearray(b"".join(qs)), dtype=torch.uint8).to(DEV)
            offs = np.zeros(len(qs) + 1, dtype=np.int64)
            np.cumsum([len(q) for q in qs], out=offs[1:])
            off = torch.from_numpy(offs).to(DEV)
            for thr in (0.3, 0.0):
                pg = pgs[step % 2]
                step += 1
                pg.batch = len(qs)  # (the buffers are sized for the larger batch, as a ragged last step)
                pg.buf[0] = len(qs)
                pg.counts = pg.buf[2:2 + pg.batch]
                gi.search_device(raw.data_ptr(), off.data_ptr(), len(qs), thr, limit, limit, pg.counts.data_ptr(),
                                 pg.keys.data_ptr(), pg.scores.data_ptr(), side.cuda_stream)
                pg.pack(packer, side.cuda_stream)
                counts, keys, scores = shard.PackedGather.decode(pg.buf, pg.pad_b, limit)
                c, k = counts.cpu().tolist(), keys.cpu().tolist()
                s = scores.view(torch.int32).cpu().numpy().view(np.uint32)
                host = gi.score_batch(qs, thr, limit)
                assert sum(c) == len(k) == int(pg.buf[1])
                if thr == 0.0:  # a query of two characters scores every key: full counts
                    assert c[:40] == [limit] * 40
                o = 0
                for i, (q, h) in enumerate(zip(qs, host)):
                    got = [(gi.key(k[o + j]), int(s[o + j])) for j in range(c[i])]
                    want = [(key, int(np.float32(sc).view(np.uint32))) for key, sc in h]
                    assert got == want, f"step {step} thr={thr} #{i} q={q!r}"
                    o += c[i]
                for i in (0, 5, len(qs) - 1):  # and scoreBatch is the oracle's answer
                    ref = oi.score(qs[i], thr, limit)
                    assert [(a, np.float32(b).tobytes()) for a, b in host[i]] == \
                           [(a, np.float32(b).tobytes()) for a, b in ref]
    gi.dispose()
