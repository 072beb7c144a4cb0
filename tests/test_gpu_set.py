"""Index sets on the GPU: ngsMergeResultsDevice over planted blocks against the model of tests/set_ref.py,
and sets of real indexes end to end against the oracle over all rows and against one index over all
rows. Every comparison is exact: key strings or ids, order, fp32 bits."""
import ctypes as C

import numpy as np
import pytest

import set_cases
import set_corpus
import set_ref
from oracle_py import OracleIndex, OracleIndexG

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64
CANARY = 0x5A5AA5A5
FILL = 0x0BADBAD0    # the output block before the merge (no planted key id or score has these bits)
CASES = set_cases.cases()
GRID = [(t, l) for t in set_corpus.THRESHOLDS for l in set_corpus.LIMITS]


def dev(a):
    """A u32 array on the device (as int32: only its address and its bits matter)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def padded(a):
    """`a` between two runs of canaries: (the whole tensor, the address of a[0])."""
    whole = np.full(len(a) + 2 * PAD, CANARY, dtype=np.uint32)
    whole[PAD:PAD + len(a)] = a
    t = dev(whole)
    return t, t.data_ptr() + 4 * PAD


def run_merge(parts, n, limit, out_stride=None):
    """ngsMergeResultsDevice on padded copies of the parts -> (counts, rows), after the checks that
    nothing outside the output block and no input changed."""
    out_stride = set_ref.min_stride(parts, limit) if out_stride is None else out_stride
    ins, desc = [], []
    for p in parts:
        held = [padded(np.asarray(p[f], dtype=np.uint32)) for f in ("counts", "keys", "scores", "lens")]
        ins.append((p, held))
        desc.append((held[0][1], held[1][1], held[2][1], p["stride"], p["base"], held[3][1], len(p["lens"])))
    fill = np.full(n * out_stride, FILL, dtype=np.uint32)
    oc, ok, os_ = padded(np.full(n, FILL, dtype=np.uint32)), padded(fill), padded(fill)
    ssl.merge_results_device(desc, n, limit, out_stride, oc[1], ok[1], os_[1])
    torch.cuda.synchronize()
    for p, held in ins:
        for f, (t, _) in zip(("counts", "keys", "scores", "lens"), held):
            h = host(t)
            assert (h[:PAD] == CANARY).all() and (h[len(h) - PAD:] == CANARY).all(), f
            assert np.array_equal(h[PAD:len(h) - PAD], np.asarray(p[f], dtype=np.uint32)), f"input {f} changed"
    got = []
    for t, _ in (oc, ok, os_):
        h = host(t)
        assert (h[:PAD] == CANARY).all() and (h[len(h) - PAD:] == CANARY).all(), "a write outside the block"
        got.append(h[PAD:len(h) - PAD])
    counts, keys, scores = got
    assert (counts <= out_stride).all()
    # a row's records are written to its first counts[i] cells and nowhere else: no row reaches into another
    for i, c in enumerate(counts.tolist()):
        for block in (keys, scores):
            assert (block[i * out_stride + c:(i + 1) * out_stride] == FILL).all(), f"row {i}: a write past its count"
    rows = [list(zip(keys[i * out_stride:i * out_stride + c].tolist(), scores[i * out_stride:i * out_stride + c].tolist()))
            for i, c in enumerate(counts.tolist())]
    return counts, rows


# ---- 1. planted blocks, no handle ---------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_merge_of_planted_blocks_equals_the_model(case):
    name, parts, n, limits = case
    assert n <= 8
    for limit in limits:
        want_c, want = set_ref.merge(parts, n, limit)
        got_c, got = run_merge(parts, n, limit)
        assert got_c.tolist() == want_c.tolist(), (name, limit)
        for i in range(n):
            assert got[i] == want[i], (name, limit, i, got[i][:4], want[i][:4])


def test_merge_with_a_roomier_stride_no_queries_and_a_repeat():
    name, parts, n, _ = next(c for c in CASES if c[0] == "uneven")
    want_c, want = set_ref.merge(parts, n, 50)
    for _ in range(2):  # reproducible bit for bit
        got_c, got = run_merge(parts, n, 50, out_stride=77)
        assert got_c.tolist() == want_c.tolist() and got == want
    got_c, got = run_merge(parts, 0, 10, out_stride=10)  # nQueries = 0: nothing is written
    assert len(got_c) == 0


# ---- sets of real indexes ---------------------------------------------------------------------------
class Lib:
    """A library cut into parts: one index per part in an IndexSet, one index over all rows, the oracle."""

    def __init__(self, cls, words, weights, cuts, oracle):
        self.words, self.cuts = words, cuts
        self.members = [cls(w, set_corpus.ROW, wt, device=0) for w, wt in set_corpus.split(words, weights, cuts)]
        self.set = ssl.IndexSet(self.members)
        self.whole = cls(words, set_corpus.ROW, weights, device=0)
        self.oracle = oracle
        self._want = {}

    def want(self, queries, thr, limit):
        """The oracle's answer over all rows, computed once per (threshold, limit)."""
        key = (id(queries), thr, limit)
        if key not in self._want:
            self._want[key] = [self.oracle.score(q, thr, limit) for q in queries]
        return self._want[key]

    def dispose(self):
        self.set.dispose()
        for m in self.members + [self.whole]:
            m.dispose()


@pytest.fixture(scope="module")
def narrow_lib():
    words, weights, cuts = set_corpus.narrow()
    lib = Lib(ssl.StringIndex, words, weights, cuts, OracleIndex(words, set_corpus.ROW, weights))
    yield lib
    lib.dispose()


def same(got, want, where):
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        gk, wk = [k for k, _ in g], [k for k, _ in w]
        assert gk == wk, f"{where}: query {i}: keys {gk[:4]} vs {wk[:4]} ({len(gk)} vs {len(wk)})"
        gs = np.array([s for _, s in g], dtype=np.float32).view(np.uint32)
        ws = np.array([s for _, s in w], dtype=np.float32).view(np.uint32)
        assert np.array_equal(gs, ws), f"{where}: query {i}: score bits differ"


def test_the_narrow_library_is_what_the_test_needs(narrow_lib):
    lib, qs = narrow_lib, set_corpus.narrow_queries()
    assert [m.num_keys() for m in lib.members][0] == 2 and len(lib.members) == 3
    assert lib.set.num_keys() == lib.whole.num_keys() == lib.oracle.n_keys() == 6000
    for thr, limit in GRID:  # no case may be skipped: the oracle's answer is unambiguous for every query
        assert not any(lib.oracle.score_amb(q, thr, limit)[1] for q in qs), (thr, limit)
    ties = lib.oracle.score(set_corpus.TIE_QUERY, 0.0, 0)
    assert sum(1 for _, s in ties if s == ties[0][1]) >= set_corpus.FAMILY
    last = set(lib.words[set_corpus.ROW * lib.cuts[2]::set_corpus.ROW])
    promoted = [q for q in qs if q in last]
    assert len(promoted) >= 20 and all(lib.oracle.score(q, 0.3, 1)[0] == (q, 100.0) for q in promoted)


# ---- 2. exact against the oracle, narrow --------------------------------------------------------------
@pytest.mark.parametrize("thr,limit", GRID)
def test_narrow_set_equals_the_oracle_and_one_index_over_all_rows(narrow_lib, thr, limit):
    lib, qs = narrow_lib, set_corpus.narrow_queries()
    got = lib.set.score_batch(qs, thr, limit)
    same(got, lib.want(qs, thr, limit), f"set vs oracle at ({thr}, {limit})")
    same(got, lib.whole.score_batch(qs, thr, limit), f"set vs one index at ({thr}, {limit})")


# ---- 3. the same, wide --------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [ssl.WideStringIndex, ssl.Utf8StringIndex], ids=["W", "U8"])
def test_wide_set_equals_the_oracle_and_one_index_over_all_rows(cls):
    words, weights, cuts = set_corpus.wide()
    lib = Lib(cls, words, weights, cuts, OracleIndexG(words, set_corpus.ROW, weights, g=2, wide=True))
    try:
        assert lib.set.num_keys() == lib.oracle.n_keys() and lib.members[0].gram_size() == 2
        qs = set_corpus.wide_queries()
        # the tie family spans both parts and is larger than every limit of the grid but 0
        ties = lib.oracle.score(set_corpus.WIDE_TIE_QUERY, 0.0, 0)
        family = {k for k, s in ties if s == ties[0][1]}
        assert len(family) >= set_corpus.WIDE_FAMILY > max(set_corpus.LIMITS)
        first = set(words[:set_corpus.ROW * cuts[1]:set_corpus.ROW])
        assert family & first and family - first
        for thr, limit in GRID:
            got = lib.set.score_batch(qs, thr, limit)
            same(got, lib.want(qs, thr, limit), f"{cls.__name__} set vs oracle at ({thr}, {limit})")
            same(got, lib.whole.score_batch(qs, thr, limit), f"{cls.__name__} set vs one index at ({thr}, {limit})")
            if limit:  # the limit cuts inside the tie class
                row = got[qs.index(set_corpus.WIDE_TIE_QUERY)]
                assert len(row) == limit and {k for k, _ in row} < family, (thr, limit)
        # the other width's host form answers 0 on this set
        L = _native.lib()
        counts = (C.c_uint32 * 1)(9)
        L.ngsLastError(1)
        assert L.scoreBatchSet(lib.set.set_id, (C.c_char_p * 1)(b"AB"), 1, 0.0, 10, 10, counts,
                               (C.c_uint32 * 10)(), (C.c_float * 10)()) == 0
        assert L.ngsLastError(1) != 0 and counts[0] == 0
    finally:
        lib.dispose()


def test_a_narrow_set_refuses_the_wide_host_forms_and_a_wide_member(narrow_lib):
    L = _native.lib()
    counts = (C.c_uint32 * 1)(9)
    q = (_native.W * 1)(C.cast((C.c_uint32 * 3)(65, 66, 0), _native.W))
    for fn, arg in ((L.scoreBatchSetW, q), (L.scoreBatchSetU8, (C.c_char_p * 1)(b"AB"))):
        L.ngsLastError(1)
        assert fn(narrow_lib.set.set_id, arg, 1, 0.0, 10, 10, counts, (C.c_uint32 * 10)(), (C.c_float * 10)()) == 0
        assert L.ngsLastError(1) != 0
    w = ssl.WideStringIndex(["abcdef", "ghijkl"], 1, None, device=0)
    g2 = ssl.StringIndex([b"abcdef", b"ghijkl"], 1, None, device=0, gram_size=2)
    try:
        for other in (w, g2):  # another width, another gram size
            assert L.ngsSetAdd(narrow_lib.set.set_id, other.handle) == -3
            hs = (C.c_uint32 * 2)(narrow_lib.members[0].handle, other.handle)
            assert L.ngsSetCreate(hs, 2) == 0
        assert L.ngsSetParts(narrow_lib.set.set_id) == 3
    finally:
        w.dispose()
        g2.dispose()


# ---- 4. append ------------------------------------------------------------------------------------------
def test_append_keeps_ids_and_equals_one_index_over_all_rows():
    words, weights, _ = ssl.synth.gen_corpus(2050, seed=91, min_len=5, span=12, row_size=set_corpus.ROW)
    cut = set_corpus.ROW * 2000
    base = ssl.StringIndex(words[:cut], set_corpus.ROW, weights[:cut], device=0)
    whole = ssl.StringIndex(words, set_corpus.ROW, weights, device=0)
    s = ssl.IndexSet([base])
    try:
        n0 = base.num_keys()
        before = [s.key(g) for g in range(n0)]
        added = s.append(words[cut:], set_corpus.ROW, weights[cut:])
        assert isinstance(added, ssl.StringIndex) and s.parts == [base, added] and added.num_keys() == 50
        assert s.num_keys() == n0 + 50 == whole.num_keys()
        assert [s.key(g) for g in range(n0)] == before
        for g in (0, n0 - 1, n0, n0 + 49):
            index, k = s.locate(g)
            assert (index is base and k == g) if g < n0 else (index is added and k == g - n0)
        with pytest.raises(IndexError):
            s.locate(n0 + 50)
        rng = ssl.synth.SplitMix64(3)
        qs = ssl.synth.gen_queries(words, set_corpus.ROW, 60, rng) + words[cut::set_corpus.ROW][:20] + [b"", b"*", b"AB"]
        for thr, limit in ((0.0, 10), (0.3, 0)):
            same(s.score_batch(qs, thr, limit), whole.score_batch(qs, thr, limit), f"append at ({thr}, {limit})")
    finally:
        s.dispose()
        for ix in s.parts + [whole]:
            ix.dispose()


# ---- 5. entry-point agreement --------------------------------------------------------------------------
def device_batch(queries):
    raw = b"".join(queries)
    off = np.cumsum([0] + [len(q) for q in queries]).astype(np.uint64)
    d_raw = torch.from_numpy(np.frombuffer(raw + b"\0" * 16, dtype=np.uint8).copy()).to(DEV)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(DEV)
    return d_raw, d_off


@pytest.mark.parametrize("thr,limit", [(0.3, 10), (0.0, 100), (0.3, 0)])
def test_entry_points_agree(narrow_lib, thr, limit):
    lib, qs, L = narrow_lib, set_corpus.narrow_queries(), _native.lib()
    nq = len(qs)
    stride = min(limit or set_ref.LIMIT_ALL, lib.set.num_keys())
    # scoreBatchSet through ctypes
    counts = np.full(nq, 9, dtype=np.uint32)
    keys = np.zeros(nq * stride, dtype=np.uint32)
    scores = np.zeros(nq * stride, dtype=np.float32)
    L.ngsLastError(1)
    total = L.scoreBatchSet(lib.set.set_id, (C.c_char_p * nq)(*qs), nq, thr, limit, stride,
                            counts.ctypes.data_as(C.POINTER(C.c_uint32)), keys.ctypes.data_as(C.POINTER(C.c_uint32)),
                            scores.ctypes.data_as(C.POINTER(C.c_float)))
    assert L.ngsLastError(1) == 0 and total == counts.sum()
    # ngsSetSearchDevice
    d_raw, d_off = device_batch(qs)
    d_n, d_k, d_s = dev(np.zeros(nq)), dev(np.zeros(nq * stride)), dev(np.zeros(nq * stride))
    lib.set.search_device(d_raw.data_ptr(), d_off.data_ptr(), nq, thr, limit, stride, d_n.data_ptr(), d_k.data_ptr(),
                          d_s.data_ptr())
    dn, dk, ds = host(d_n), host(d_k), host(d_s)
    assert np.array_equal(dn, counts)
    py = lib.set.score_batch(qs, thr, limit)
    sb = scores.view(np.uint32)
    for i in range(nq):
        c, at = int(counts[i]), i * stride
        assert np.array_equal(dk[at:at + c], keys[at:at + c]) and np.array_equal(ds[at:at + c], sb[at:at + c]), i
        assert [k for k, _ in py[i]] == [lib.set.key(int(g)) for g in keys[at:at + c]], i
        assert np.array_equal(np.array([s for _, s in py[i]], dtype=np.float32).view(np.uint32), sb[at:at + c]), i
    # a stride below min(L, keys) is refused
    if stride > 1:
        assert L.ngsSetSearchDevice(lib.set.set_id, d_raw.data_ptr(), d_off.data_ptr(), nq, thr, limit, stride - 1,
                                    d_n.data_ptr(), d_k.data_ptr(), d_s.data_ptr(), None) == -3


# ---- 6. a disposed member -------------------------------------------------------------------------------
def test_a_disposed_member_fails_the_set_until_it_is_disposed():
    L = _native.lib()
    words, weights, _ = ssl.synth.gen_corpus(300, seed=17, min_len=5, span=8)
    members = [ssl.StringIndex(words[a:b], 1, weights[a:b], device=0) for a, b in ((0, 100), (100, 200), (200, 300))]
    s = ssl.IndexSet(members)
    fresh = None
    try:
        qs = [words[5], words[150], words[250]]
        assert [r[0] for r in s.score_batch(qs, 0.3, 1)] == [(q, 100.0) for q in qs]
        d_raw, d_off = device_batch(qs)
        d_n, d_k, d_s = dev(np.zeros(3)), dev(np.zeros(30)), dev(np.zeros(30))

        def search():
            return L.ngsSetSearchDevice(s.set_id, d_raw.data_ptr(), d_off.data_ptr(), 3, 0.3, 10, 10, d_n.data_ptr(),
                                        d_k.data_ptr(), d_s.data_ptr(), None)

        def batch():
            counts = (C.c_uint32 * 3)(9, 9, 9)
            L.ngsLastError(1)
            got = L.scoreBatchSet(s.set_id, (C.c_char_p * 3)(*qs), 3, 0.3, 10, 10, counts, (C.c_uint32 * 30)(),
                                  (C.c_float * 30)())
            return got, L.ngsLastError(1), list(counts)

        assert search() == 0
        freed = members[1].handle
        members[1].dispose()
        for again in range(2):
            assert search() == -1
            got, err, counts = batch()
            assert got == 0 and err != 0 and counts == [0, 0, 0]
            assert L.ngsSetParts(s.set_id) == -1 and L.ngsSetNumKeys(s.set_id) == 0
            assert L.ngsSetLocate(s.set_id, 0, None, None) == -1 and L.ngsSetAdd(s.set_id, members[0].handle) == -1
            if fresh is None:  # a fresh index takes the freed handle id: the set is not fooled
                fresh = ssl.StringIndex(words[100:200], 1, weights[100:200], device=0)
                assert fresh.handle == freed
        sid = s.set_id
        s.dispose()
        assert L.ngsSetParts(sid) == -1 and search() == -1
        for m, q in ((members[0], qs[0]), (members[2], qs[2]), (fresh, qs[1])):
            assert m.score_batch([q], 0.3, 1) == [[(q, 100.0)]]
    finally:
        s.dispose()
        for m in members + [fresh]:
            if m is not None:
                m.dispose()


# ---- 7. ngsKeyLengthsDevice ---------------------------------------------------------------------------
def check_lengths(index):
    nk = index.num_keys()
    want = np.array([len(index.key(k)) for k in range(nk)], dtype=np.uint32)
    for first, count in ((0, nk), (0, 0), (nk, 0), (nk // 3, nk // 2), (nk - 1, 1), (nk - min(nk, 70), min(nk, 70))):
        t, at = padded(np.zeros(count, dtype=np.uint32))
        index.key_lengths_device(first, count, at)
        torch.cuda.synchronize()
        h = host(t)
        assert (h[:PAD] == CANARY).all() and (h[PAD + count:] == CANARY).all()
        assert np.array_equal(h[PAD:PAD + count], want[first:first + count]), (first, count)
    assert _native.lib().ngsKeyLengthsDevice(index.handle, nk, 1, 0x1000, None) == -3
    assert _native.lib().ngsKeyLengthsDevice(index.handle, 0xFFFFFFFF, 2, 0x1000, None) == -3


def test_key_lengths_equal_the_keys(narrow_lib):
    for m in narrow_lib.members:
        check_lengths(m)
    words, weights, cuts = set_corpus.wide()
    w = ssl.WideStringIndex(words[:2 * cuts[1]], set_corpus.ROW, weights[:2 * cuts[1]], device=0)
    try:
        check_lengths(w)
    finally:
        w.dispose()
