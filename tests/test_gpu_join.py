"""The self-join on the GPU: the gather of the keys as a query batch, drop-self and the union-find on
fabricated blocks, the join against the oracle (tests/join_ref.py) and dedup end to end.
Every comparison is exact: counts, key ids in order, fp32 bits, labels."""
import collections
import ctypes as C
import random

import numpy as np
import pytest

import join_cases
import join_ref
import sim_ref
from oracle_py import OracleIndex, OracleIndexG

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
FILL32 = 0x5A5AA5A5
SETTINGS = [(0.0, 0), (0.5, 11), (0.3, 1), (1.0, 5)]
NGS_ERR_RERANK_LIMIT = 0x10003
HIP_INVALID_VALUE = 1


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.current_stream().synchronize()


# ---- gather ----------------------------------------------------------------------------------
def key_units(ix, k, cs):
    s = ix.key(k)
    return np.frombuffer(s, dtype=np.uint8) if cs == 1 else np.array([ord(c) for c in s], dtype="<u4").view(np.uint8)


def check_gather(ix, cs, first, n, shift=0):
    """ngsKeyQueriesDevice of keys [first, first + n) into a buffer `shift` bytes off its allocation."""
    want = np.concatenate([key_units(ix, first + i, cs) for i in range(n)] + [np.zeros(0, dtype=np.uint8)])
    want_off = join_ref.query_offsets([len(key_units(ix, first + i, cs)) // cs for i in range(n)], cs)
    total = ix.key_query_bytes(first, n)
    assert total == len(want) == want_off[-1]
    buf = torch.full((shift + total + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    off = torch.full((n + 1 + GUARD,), -7, dtype=torch.int64, device=DEV)
    sync()
    ix.key_queries_device(first, n, buf.data_ptr() + shift, total, off.data_ptr(), stream())
    sync()
    b, o = buf.cpu().numpy(), off.cpu().numpy()
    where = f"cs={cs} first={first} n={n} shift={shift}"
    assert o[:n + 1].tolist() == want_off, where
    assert (o[n + 1:] == -7).all(), f"{where}: offsets written past n + 1"
    assert np.array_equal(b[shift:shift + total], want), f"{where}: first bad byte {np.flatnonzero(b[shift:shift + total] != want)[:1]}"
    assert (b[:shift] == 0xA5).all() and (b[shift + total:] == 0xA5).all(), f"{where}: wrote outside the capacity"
    return total


def test_gather_narrow():
    rng = random.Random(31)
    word = lambda n: bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 .") for _ in range(n - 2)).join([b"Q", b"Z"])
    lens = [3, 4, 15, 16, 17, 63, 64, 65, 300]
    words = [b"K", b"PW", b"*", b"###", b" a b "] + [word(n) for n in lens] + [word(rng.randint(3, 40)) for _ in range(60)]
    rng.shuffle(words)
    ix = ssl.StringIndex(words)
    nk = ix.num_keys()
    keys = [ix.key(k) for k in range(nk)]
    assert {len(k) for k in keys} >= {1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 300}
    assert {b"*", b"###", b"a b"} <= set(keys)
    for first, n in ((0, nk), (nk - 1, 1), (5, 0), (3, nk - 3), (7, 11), (nk, 0)):
        for shift in (0, 1, 13):
            check_gather(ix, 1, first, n, shift)
    # a capacity one byte short, a range past the keys
    L = _native.lib()
    total = ix.key_query_bytes(0, nk)
    buf = torch.zeros(total + 16, dtype=torch.uint8, device=DEV)
    off = torch.zeros(nk + 2, dtype=torch.int64, device=DEV)
    assert L.ngsKeyQueriesDevice(ix.handle, 0, nk, buf.data_ptr(), total - 1, off.data_ptr(), None) == -3
    assert L.ngsKeyQueriesDevice(ix.handle, 1, nk, buf.data_ptr(), total, off.data_ptr(), None) == -3
    assert L.ngsKeyQueriesDevice(ix.handle, nk + 1, 0, buf.data_ptr(), total, off.data_ptr(), None) == -3
    assert ix.key_query_bytes(1, nk) == 0 and ix.key_query_bytes(nk, 0) == 0
    ix.dispose()


def test_gather_wide():
    rng = random.Random(32)
    alpha = "ABCDEFGHIJ abc 0123 éßÖ 日本語 \U0001F600\U00020000\U0010FFFF"
    words = ["".join(rng.choice(alpha) for _ in range(n)).strip() or "X" for n in [1, 2, 3, 4, 5, 16, 17, 64, 65, 130] * 4]
    words += ["\U0001F600", "\U00020000\U0010FFFF"]
    ix = ssl.WideStringIndex(words, gram_size=2)
    nk = ix.num_keys()
    assert any(ord(c) > 0xFFFF for k in range(nk) for c in ix.key(k))
    for first, n in ((0, nk), (nk - 1, 1), (5, 0), (3, nk - 3)):
        for shift in (0, 4, 12):
            check_gather(ix, 4, first, n, shift)
    L = _native.lib()
    total = ix.key_query_bytes(0, nk)
    buf = torch.zeros(total + 16, dtype=torch.uint8, device=DEV)
    off = torch.zeros(nk + 2, dtype=torch.int64, device=DEV)
    assert L.ngsKeyQueriesDevice(ix.handle, 0, nk, buf.data_ptr(), total - 1, off.data_ptr(), None) == -3
    assert L.ngsKeyQueriesDevice(ix.handle, 0, nk, buf.data_ptr() + 2, total, off.data_ptr(), None) == -3  # UTF-32 units
    ix.dispose()


# ---- drop-self on fabricated blocks ----------------------------------------------------------------
@pytest.mark.parametrize("stride", join_cases.DROP_STRIDES)
def test_drop_self_on_fabricated_blocks(stride):
    counts, keys, scores = join_cases.drop_block(stride)
    n = len(counts)
    guard_k = np.full(GUARD, FILL32, dtype=np.uint32)
    for limit in join_cases.drop_limits(stride):
        dn = dev_u32(np.concatenate([counts, guard_k]))
        dk = dev_u32(np.concatenate([keys, guard_k]))
        ds = dev_u32(np.concatenate([scores.view(np.uint32), guard_k])).view(torch.float32)
        sync()
        ssl.StringIndex.drop_self_device(dn.data_ptr(), dk.data_ptr(), ds.data_ptr(), n, stride, join_cases.DROP_FIRST,
                                         limit, stream())
        sync()
        gn, gk, gs = host_u32(dn), host_u32(dk), host_u32(ds.view(torch.int32))
        assert (gn[n:] == FILL32).all() and (gk[n * stride:] == FILL32).all() and (gs[n * stride:] == FILL32).all(), \
            f"stride {stride} limit {limit}: wrote past the block"
        for i in range(n):
            a = i * stride
            kept, wk, ws = join_ref.drop_self(keys[a:a + stride], scores[a:a + stride].view(np.uint32), int(counts[i]),
                                              stride, join_cases.DROP_FIRST + i, limit)
            where = f"stride {stride} limit {limit} row {i} (count {counts[i]})"
            assert gn[i] == kept, where
            assert gk[a:a + kept].tolist() == wk, where
            assert gs[a:a + kept].tolist() == ws, f"{where}: a score left its key"


# ---- the join against the oracle -------------------------------------------------------------------
class Lib:
    """An index, its oracle and the map between their key ids; the expected joins are computed once
    per threshold and shared."""

    def __init__(self, ix, oi):
        self.ix, self.oi = ix, oi
        self.nk = ix.num_keys()
        assert self.nk == oi.n_keys()
        self.keys = [ix.key(k) for k in range(self.nk)]
        gid = {s: k for k, s in enumerate(self.keys)}
        assert len(gid) == self.nk
        self.omap = np.array([gid[oi.key(k)] for k in range(self.nk)], dtype=np.uint32)
        self._rows = {}

    def rows(self, thr, limit, valid=None):
        if (thr, limit, valid) not in self._rows:
            self._rows.update({(thr, lim, valid): r for lim, r in join_ref.oracle_join(
                self.oi, self.keys, self.omap, 0, self.nk, thr, sorted({limit} | {l for t, l in SETTINGS if t == thr})).items()})
        return self._rows[(thr, limit, valid)]

    def stride(self, limit):
        return min((limit or 2**31 - 1) + 1, self.nk)

    def join_device(self, first, n, thr, limit):
        """ngsSelfJoinDevice -> (counts, keys [n][stride], score bits [n][stride])."""
        st = self.stride(limit)
        dn = torch.full((n + GUARD,), -3, dtype=torch.int32, device=DEV)
        dk = torch.full((n * st + GUARD,), -3, dtype=torch.int32, device=DEV)
        ds = torch.full((n * st + GUARD,), -3, dtype=torch.int32, device=DEV)
        sync()
        self.ix.self_join_device(first, n, thr, limit, st, dn.data_ptr(), dk.data_ptr(), ds.data_ptr(), stream())
        gn, gk, gs = host_u32(dn), host_u32(dk), host_u32(ds)  # (complete on return: no sync of ours)
        assert (gn[n:] == 0xFFFFFFFD).all() and (gk[n * st:] == 0xFFFFFFFD).all() and (gs[n * st:] == 0xFFFFFFFD).all()
        return gn[:n], gk[:n * st].reshape(n, st), gs[:n * st].reshape(n, st)


def check_rows(got, want, where, first=0):
    gn, gk, gs = got
    assert len(gn) == len(want)
    for i, (wk, ws) in enumerate(want):
        c = len(wk)
        assert gn[i] == c, f"{where}: key {first + i}: {gn[i]} records, the oracle {c}"
        assert np.array_equal(gk[i][:c], wk), f"{where}: key {first + i}: ids {gk[i][:c][:6]} vs {wk[:6]}"
        assert np.array_equal(gs[i][:c], ws), f"{where}: key {first + i}: score bits differ"


def rows_corpus():
    """The "rows" corpus of test_gpu_parity.py: aliases, NULL holes, zero / negative weights, duplicate keys."""
    words, wts, _ = ssl.synth.gen_corpus(3000, seed=9, min_len=3, span=12, row_size=3)
    words = list(words)
    for i in range(0, len(words), 29):
        words[i] = None
    for i in range(7, len(words), 31):
        words[i] = words[i - 6]
    for i in range(2, len(wts), 17):
        wts[i] = 0.0
    for i in range(4, len(wts), 19):
        wts[i] = -0.75
    return words, 3, wts


@pytest.fixture(scope="module")
def rows_lib():
    words, rs, wts = rows_corpus()
    lib = Lib(ssl.StringIndex(words, rs, wts), OracleIndex(words, rs, wts))
    yield lib
    lib.ix.dispose()


@pytest.fixture(scope="module")
def short_lib():
    words, _, _ = ssl.synth.gen_corpus(6000, seed=4, min_len=1, span=9)
    lib = Lib(ssl.StringIndex(words), OracleIndex(words))
    yield lib
    lib.ix.dispose()


def test_rows_corpus_meets_every_branch_of_drop_self(rows_lib):
    """Properties of the oracle's join alone: real search output has rows without the key's own record,
    rows where it is not first, and full rows."""
    assert rows_lib.nk == 2803
    for thr, absent, not_first in ((0.0, 110, 41), (0.5, 150, 1)):
        full = join_ref.oracle_full(rows_lib.oi, rows_lib.keys, thr)
        ids = [rows_lib.omap[k] if len(k) else k for k, _ in full]
        assert sum(1 for i, k in enumerate(ids) if i not in k) == absent
        assert sum(1 for i, k in enumerate(ids) if i in k and k[0] != i) == not_first
    assert sum(1 for k, _ in rows_lib.rows(0.5, 11) if len(k) == 11) == 448


@pytest.mark.parametrize("thr,limit", SETTINGS)
def test_join_rows_corpus(rows_lib, thr, limit):
    check_rows(rows_lib.join_device(0, rows_lib.nk, thr, limit), rows_lib.rows(thr, limit), f"rows thr={thr} limit={limit}")


@pytest.mark.parametrize("thr,limit", [(0.0, 12), (0.5, 11)])
def test_join_short_corpus(short_lib, thr, limit):
    """Queries of <= 3 characters scan the whole library, <= 8 go through the Levenshtein path."""
    assert short_lib.nk == 5143
    check_rows(short_lib.join_device(0, short_lib.nk, thr, limit), short_lib.rows(thr, limit),
               f"short thr={thr} limit={limit}")


def test_join_wide_corpus():
    rng = random.Random(33)
    alpha = "ABCDEFGHIJKLMNOP" "abcdxyz" "0123456789" "  " "éßÖçñ" "日本語中文字" "テキスト" "\U0001F600\U00020000"
    words = ["".join(rng.choice(alpha) for _ in range(rng.randint(1, 24))) for _ in range(400)]
    wts = [rng.choice([1.0, 0.5, 2.0, 0.0, -0.5, 0.75]) for _ in words]
    lib = Lib(ssl.WideStringIndex(words, 1, wts, gram_size=2), OracleIndexG(words, 1, wts, g=2, wide=True))
    assert 200 < lib.nk <= 400
    for thr, limit in SETTINGS:
        check_rows(lib.join_device(0, lib.nk, thr, limit), lib.rows(thr, limit), f"wide thr={thr} limit={limit}")
    lib.ix.dispose()


def test_three_entry_points_agree(rows_lib):
    lib, ix, nk = rows_lib, rows_lib.ix, rows_lib.nk
    thr, limit = 0.5, 11
    want = lib.rows(thr, limit)
    # ngsSelfJoinDevice on sub-ranges
    for first, n in ((0, 1), (1000, 803), (nk - 1, 1), (5, 0), (nk, 0), (1, nk - 1)):
        check_rows(lib.join_device(first, n, thr, limit), want[first:first + n], f"range ({first}, {n})", first)
    L = _native.lib()
    st = lib.stride(limit)
    dn = torch.zeros(8, dtype=torch.int32, device=DEV)
    dk = torch.zeros(8 * st, dtype=torch.int32, device=DEV)
    ds = torch.zeros(8 * st, dtype=torch.float32, device=DEV)
    args = (dn.data_ptr(), dk.data_ptr(), ds.data_ptr(), None)
    assert L.ngsSelfJoinDevice(ix.handle, 0, 8, thr, limit, st - 1, *args) == -3  # one less than limit + 1
    assert L.ngsSelfJoinDevice(ix.handle, nk - 7, 8, thr, limit, st, *args) == -3  # past the keys
    assert L.ngsSelfJoinDevice(ix.handle, 0, 8, thr, limit, st, *args) == 0
    # selfJoin into caller-allocated arrays, at the smallest stride and a larger one
    for stride in (limit, limit + 5):
        counts = np.full(nk, 99, dtype=np.uint32)
        keys = np.zeros(nk * stride, dtype=np.uint32)
        scores = np.zeros(nk * stride, dtype=np.uint32)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        total = L.selfJoin(ix.handle, 0, nk, thr, limit, stride, p(counts, C.c_uint32), p(keys, C.c_uint32),
                           p(scores, C.c_float))
        assert total == sum(len(k) for k, _ in want) == int(counts.sum())
        check_rows((counts, keys.reshape(nk, stride), scores.reshape(nk, stride)), want, f"selfJoin stride {stride}")
    counts = np.full(nk, 99, dtype=np.uint32)
    L.ngsLastError(1)
    assert L.selfJoin(ix.handle, 0, nk, thr, limit, limit - 1, p(counts, C.c_uint32), p(keys, C.c_uint32),
                      p(scores, C.c_float)) == 0
    assert not counts.any() and L.ngsLastError(1) == HIP_INVALID_VALUE
    # self_join, whole and a range
    py = ix.self_join(threshold=thr, limit=limit)
    assert len(py) == nk
    for i, (wk, ws) in enumerate(want):
        assert [k for k, _ in py[i]] == wk.tolist() and [int(np.float32(s).view(np.uint32)) for _, s in py[i]] == ws.tolist()
    assert ix.self_join(100, 50, thr, limit) == py[100:150]
    # score_batch of the key strings at limit + 1, the key's own record dropped on the host
    for a in range(0, nk, 1024):
        got = ix.score_batch(lib.keys[a:a + 1024], thr, limit + 1)
        for i, g in enumerate(got, a):
            row = [(k, s) for k, s in g if k != lib.keys[i]][:limit]
            assert [(lib.keys[k], s) for k, s in py[i]] == row, f"key {i}"


def test_join_follows_the_valid_char_set():
    words, wts, _ = ssl.synth.gen_corpus(1500, seed=12)
    lib = Lib(ssl.StringIndex(words, 1, wts), OracleIndex(words, 1, wts))
    for valid in (b"ABCDEF ", b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"):
        lib.ix.set_valid_char(valid)
        lib.oi.set_valid_char(valid)
        check_rows(lib.join_device(0, lib.nk, 0.2, 5), lib.rows(0.2, 5, valid), f"valid={valid[:8]!r}")
    assert any(len(a[0]) != len(b[0]) or (a[0] != b[0]).any()
               for a, b in zip(lib.rows(0.2, 5, b"ABCDEF "), lib.rows(0.2, 5, b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ")))
    lib.ix.dispose()


# ---- cluster on fabricated blocks ------------------------------------------------------------------
def run_cluster(n_labels, parts):
    """parts: [(counts, keys, n, stride, first, init, finish)] queued in order on one stream -> labels."""
    dl = torch.full((n_labels + GUARD,), -9, dtype=torch.int32, device=DEV)
    held = []
    sync()
    for counts, keys, n, stride, first, init, finish in parts:
        dn, dk = dev_u32(counts), dev_u32(keys)
        held += [dn, dk]
        sync()
        ssl.StringIndex.cluster_device(dn.data_ptr() if n else 0, dk.data_ptr() if n else 0, n, stride, first,
                                       dl.data_ptr(), n_labels, init, finish, stream())
    sync()
    out = host_u32(dl)
    assert (out[n_labels:] == 0xFFFFFFF7).all(), "labels written past nLabels"
    return out[:n_labels].tolist()


CLUSTER_CASES = join_cases.cluster_cases()


@pytest.mark.parametrize("case", CLUSTER_CASES, ids=[c[0] for c in CLUSTER_CASES])
def test_cluster_on_fabricated_blocks(case):
    name, n_labels, first, n, stride, counts, keys = case
    want = join_ref.labels(n_labels, join_ref.block_edges(counts, keys, n, stride, first))
    assert len(set(want)) < n_labels or n_labels == 1, "the case merges nothing"
    # one call
    assert run_cluster(n_labels, [(counts, keys, n, stride, first, True, True)]) == want
    # three calls: INIT on the first, FINISH on the last (the middle block is empty when n < 3)
    cuts = [0, n // 3, 2 * n // 3, n]
    parts = [(counts[a:b], keys[a * stride:b * stride], b - a, stride, first + a, j == 0, j == 2)
             for j, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    assert run_cluster(n_labels, parts) == want
    # the rows in another order (blocks of rows queued shuffled, INIT and FINISH in calls without
    # rows) and the records of every row shuffled
    rng = random.Random(n)
    k2 = keys.reshape(n, stride).copy()
    for i in range(n):
        c = min(int(counts[i]), stride)
        k2[i, :c] = rng.sample(k2[i, :c].tolist(), c)
    cuts = sorted({0, n} | {rng.randrange(n + 1) for _ in range(6)})
    blocks = list(zip(cuts, cuts[1:]))
    rng.shuffle(blocks)
    empty = np.zeros(0, dtype=np.uint32)
    parts = [(empty, empty, 0, stride, 0, True, False)]
    parts += [(counts[a:b], k2[a:b].reshape(-1), b - a, stride, first + a, False, False) for a, b in blocks]
    parts += [(empty, empty, 0, stride, 0, False, True)]
    assert run_cluster(n_labels, parts) == want


def test_cluster_without_finish_is_a_forest():
    name, n_labels, first, n, stride, counts, keys = CLUSTER_CASES[0]
    forest = run_cluster(n_labels, [(counts, keys, n, stride, first, True, False)])
    assert all(p <= k for k, p in enumerate(forest))
    roots = {k for k, p in enumerate(forest) if p == k}
    assert roots == {0}  # the chain is one component


# ---- dedup end to end ------------------------------------------------------------------------------
def planted_corpus():
    """5,000 synthetic words plus 1-3 single-substitution variants of 600 of them."""
    base, _, _ = ssl.synth.gen_corpus(5000, seed=3)
    rng = random.Random(3)
    out = list(base)
    for i in rng.sample(range(5000), 600):
        for _ in range(rng.randint(1, 3)):
            w = bytearray(base[i])
            w[rng.randrange(len(w))] = rng.choice(ssl.synth.ALPHABET)
            out.append(bytes(w))
    return out


def dedup_c(ix, thr, limit, min_sim, batch_keys):
    """dedupKeys through ctypes -> (clusters, labels)."""
    labels = np.full(ix.num_keys(), 0xFFFFFFFF, dtype=np.uint32)
    n = _native.lib().dedupKeys(ix.handle, thr, limit, min_sim, batch_keys, labels.ctypes.data_as(C.POINTER(C.c_uint32)))
    return n, labels.tolist()


def test_dedup_planted_corpus():
    words = planted_corpus()
    lib = Lib(ssl.StringIndex(words), OracleIndex(words))
    ix, nk = lib.ix, lib.nk
    rows = lib.rows(0.5, 10)
    want = join_ref.labels(nk, join_ref.rows_edges(rows))
    sizes = collections.Counter(want)
    # this construction under the oracle: keys, clusters, clusters of more than one key
    assert (nk, len(sizes), sum(1 for v in sizes.values() if v > 1)) == (6153, 4997, 593)
    for batch_keys in (0, 1000, 1):
        n, labels = dedup_c(ix, 0.5, 10, -1.0, batch_keys)
        assert n == len(sizes) and labels == want, f"batchKeys {batch_keys}"
    assert ix.dedup(0.5, 10) == want
    # min_similarity 0.9: the edges whose similarity (the key's string as the query, the other key's term) passes
    term = {k: sim_ref.normalise(s) for k, s in enumerate(lib.keys)}
    edges = join_ref.rows_edges(rows)
    sims = sim_ref.record_sims([(tuple(lib.keys[a]), {term[b]}) for a, b in edges])
    kept = [e for e, v in zip(edges, sims) if not (v < np.float32(0.9))]
    assert 0 < len(kept) < len(edges)
    want9 = join_ref.labels(nk, kept)
    assert ix.dedup(0.5, 10, min_similarity=0.9) == want9
    n, labels = dedup_c(ix, 0.5, 10, 0.9, 1000)
    assert labels == want9 and n == len(set(want9))
    ix.dispose()


def test_dedup_short_corpus(short_lib):
    """One component of 3,947 of the 5,143 keys: deep trees and contended roots."""
    want = join_ref.labels(short_lib.nk, join_ref.rows_edges(short_lib.rows(0.5, 10)))
    assert collections.Counter(want).most_common(1)[0][1] == 3947
    n, labels = dedup_c(short_lib.ix, 0.5, 10, -1.0, 0)
    assert labels == want and n == len(set(want))
    assert dedup_c(short_lib.ix, 0.5, 10, -1.0, 700)[1] == want


def test_dedup_failures(short_lib):
    ix, L = short_lib.ix, _native.lib()
    for limit, min_sim, err in ((0, -1.0, HIP_INVALID_VALUE), (4097, -1.0, NGS_ERR_RERANK_LIMIT),
                                (10, float("nan"), HIP_INVALID_VALUE)):
        L.ngsLastError(1)
        n, labels = dedup_c(ix, 0.5, limit, min_sim, 0)
        assert n == 0 and L.ngsLastError(1) == err and set(labels) == {0xFFFFFFFF}
    with pytest.raises(ValueError):
        ix.dedup(0.5, 4097)
    with pytest.raises(RuntimeError):
        ix.dedup(0.5, 0)
    n, labels = dedup_c(ix, 0.5, 4096, -1.0, 0)  # the largest limit: a stride of 4,097
    assert n == len(set(labels)) and all(p <= k for k, p in enumerate(labels))
