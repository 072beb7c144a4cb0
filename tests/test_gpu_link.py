"""linkKeys / StringIndex.link on the GPU, end to end against the model of tests/match_ref.py (the
oracle's rows, the reference similarities, the sequential greedy). Every comparison is exact: the
match, the fp32 bits of the chosen records' scores and similarities, the number of matched keys."""
import ctypes as C
import random

import numpy as np
import pytest

import match_ref
import sim_ref
import token_ref
from oracle_py import OracleIndex, OracleIndexG

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NO_MATCH = match_ref.NO_MATCH
METRIC = {"levenshtein": 0, "osa": 1}
MINUS_ONE = int(np.float32(-1.0).view(np.uint32))
# (threshold, limit, (metric, min_similarity) or None)
SETTINGS = [(0.5, 10, None), (0.5, 10, ("levenshtein", 0.9)), (0.3, 3, ("osa", 0.8))]
BATCHES = (0, 37, 1)


def link_words():
    """T: 2,000 synthetic words of 4..11 characters (short enough that unrelated words are candidates too).
    S: 1-3 single-substitution variants of each of 400 of them, 50 exact copies and 200 unrelated words."""
    t, _, _ = ssl.synth.gen_corpus(2000, seed=21, min_len=4, span=8)
    rng = random.Random(21)
    s = []
    for i in rng.sample(range(2000), 400):
        for _ in range(rng.randint(1, 3)):
            w = bytearray(t[i])
            w[rng.randrange(len(w))] = rng.choice(ssl.synth.ALPHABET)
            s.append(bytes(w))
    s += [t[i] for i in rng.sample(range(2000), 50)]
    s += ssl.synth.gen_corpus(200, seed=99, min_len=4, span=8)[0]
    rng.shuffle(s)
    return s, t


class Pair:
    """A source index, a target index and the target's oracle; the model's rows, similarities and links
    are computed once per setting and shared."""

    def __init__(self, s_ix, t_ix, t_oracle, wide=False):
        self.s, self.t, self.oi, self.wide = s_ix, t_ix, t_oracle, wide
        self.ns, self.nt = s_ix.num_keys(), t_ix.num_keys()
        assert self.nt == t_oracle.n_keys()
        self.src = [s_ix.key(a) for a in range(self.ns)]
        t_keys = [t_ix.key(b) for b in range(self.nt)]
        gid = {k: b for b, k in enumerate(t_keys)}
        assert len(gid) == self.nt
        self.omap = np.array([gid[t_oracle.key(k)] for k in range(self.nt)], dtype=np.uint32)
        self.terms = {b: {sim_ref.normalise(sim_ref.units(k, wide), sim_ref.DEFAULT_VALID, wide)}
                      for b, k in enumerate(t_keys)}
        self._rows, self._sims, self._want = {}, {}, {}

    def rows(self, thr, limit, valid=None):
        key = (thr, limit, valid)
        if key not in self._rows:
            self._rows[key] = match_ref.link_rows(self.oi, self.src, self.omap, thr, limit)
        return self._rows[key]

    def sims(self, thr, limit, metric, valid=None):
        key = (thr, limit, metric, valid)
        if key not in self._sims:
            self._sims[key] = match_ref.row_sims(self.rows(thr, limit, valid), self.src, self.terms, metric,
                                                 sim_ref.DEFAULT_VALID if valid is None else valid, self.wide)
        return self._sims[key]

    def want(self, thr, limit, filt, one_to_one, valid=None, token_sort=False):
        """(match, score bits, sim bits, edges kept) of the model."""
        key = (thr, limit, filt, one_to_one, valid, token_sort)
        if key not in self._want:
            rows = self.rows(thr, limit, valid)
            if filt is None:
                self._want[key] = match_ref.link(rows, self.nt, one_to_one=one_to_one)
            else:
                m = METRIC[filt[0]] | (match_ref.TOKEN_SORT if token_sort else 0)
                self._want[key] = match_ref.link(rows, self.nt, self.sims(thr, limit, m, valid), filt[1], one_to_one)
        return self._want[key]

    def dispose(self):
        self.s.dispose()
        if self.t is not self.s:
            self.t.dispose()


def link_c(pair, thr, limit, filt, mode, batch_keys, token_sort=False):
    """linkKeys through ctypes -> (return value, match, score bits, sim bits)."""
    n = pair.ns
    match = np.full(n, 0x77777777, dtype=np.uint32)
    scores = np.full(n, 9.0, dtype=np.float32)
    sims = np.full(n, 9.0, dtype=np.float32)
    metric = (METRIC[filt[0]] if filt else 0) | (0x100 if token_sort else 0)
    L = _native.lib()
    L.ngsLastError(1)
    got = L.linkKeys(pair.s.handle, pair.t.handle, thr, limit, metric, filt[1] if filt else -1.0, mode, batch_keys,
                     match.ctypes.data_as(C.POINTER(C.c_uint32)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                     sims.ctypes.data_as(C.POINTER(C.c_float)))
    assert L.ngsLastError(1) == 0
    return got, match, scores.view(np.uint32), sims.view(np.uint32)


def check(got, want, where):
    n, match, score, sim = got
    wm, ws, wv, _ = want
    bad = np.flatnonzero(match != wm)
    assert bad.size == 0, f"{where}: match differs at source keys {bad[:5]}: {match[bad[:5]]} vs {wm[bad[:5]]}"
    assert np.array_equal(score, ws), f"{where}: score bits differ at {np.flatnonzero(score != ws)[:5]}"
    assert np.array_equal(sim, wv), f"{where}: similarity bits differ at {np.flatnonzero(sim != wv)[:5]}"
    assert n == int((wm != NO_MATCH).sum()), where


def check_both_paths(pair, thr, limit, filt, batches=BATCHES, valid=None, token_sort=False):
    for one_to_one in (False, True):
        want = pair.want(thr, limit, filt, one_to_one, valid, token_sort)
        for bk in batches:
            where = f"thr={thr} limit={limit} filter={filt} one_to_one={one_to_one} batch_keys={bk}"
            check(link_c(pair, thr, limit, filt, int(one_to_one), bk, token_sort), want, "linkKeys " + where)
            m, sc, sv = pair.s.link(pair.t, thr, limit, None if filt is None else filt[1],
                                    filt[0] if filt else "levenshtein", token_sort, one_to_one, bk)
            assert (sv is None) == (filt is None)
            assert m.dtype == np.uint32 and sc.dtype == np.float32 and len(m) == len(sc) == pair.ns
            sv = np.full(pair.ns, -1.0, dtype=np.float32) if sv is None else sv
            check((int((m != NO_MATCH).sum()), m, sc.view(np.uint32), sv.view(np.uint32)), want, "link() " + where)


@pytest.fixture(scope="module")
def pair():
    s, t = link_words()
    p = Pair(ssl.StringIndex(s), ssl.StringIndex(t), OracleIndex(t))
    yield p
    p.dispose()


def test_the_model_alone_meets_the_conditions(pair):
    """Nothing below can pass vacuously: the two modes differ, a key stays unmatched, the filter drops some
    edges and keeps others."""
    assert pair.nt > 1900 and pair.ns > 900
    for thr, limit, filt in SETTINGS:
        best, one = pair.want(thr, limit, filt, False), pair.want(thr, limit, filt, True)
        assert int((best[0] != one[0]).sum()) >= 10, (thr, limit, filt)
        assert int((one[0] == NO_MATCH).sum()) >= 1 and int((one[0] != NO_MATCH).sum()) >= 100
        taken = one[0][one[0] != NO_MATCH]
        assert len(set(taken.tolist())) == len(taken)           # one-to-one
        shared = best[0][best[0] != NO_MATCH]
        assert len(set(shared.tolist())) < len(shared)           # best: a target chosen by several
        if filt:
            assert 0 < one[3] < pair.want(thr, limit, None, True)[3]
            assert (one[2][one[0] != NO_MATCH] != MINUS_ONE).all() and (one[2][one[0] == NO_MATCH] == MINUS_ONE).all()
        else:
            assert (one[2] == MINUS_ONE).all()
        assert (one[1][one[0] == NO_MATCH] == 0).all() and (one[1][one[0] != NO_MATCH] != 0).all()
    # without a filter, keys that lose their first choice fall to another one
    best, one = pair.want(0.5, 10, None, False), pair.want(0.5, 10, None, True)
    assert int(((one[0] != NO_MATCH) & (one[0] != best[0])).sum()) >= 20


@pytest.mark.parametrize("thr,limit,filt", SETTINGS, ids=["scores", "levenshtein-0.9", "osa-0.8"])
def test_link_matches_the_model(pair, thr, limit, filt):
    check_both_paths(pair, thr, limit, filt)


def test_link_an_index_to_itself(pair):
    """S and T one handle: no record is dropped, so every key finds itself first."""
    p = Pair(pair.t, pair.t, pair.oi)
    for one_to_one in (False, True):
        want = p.want(0.5, 10, None, one_to_one)
        assert (want[0] == np.arange(p.ns)).all()
        check(link_c(p, 0.5, 10, None, int(one_to_one), 500), want, f"self one_to_one={one_to_one}")


def test_token_sort_links_reordered_names():
    rng = random.Random(77)
    names = token_ref.reorder_pairs(rng, 120)
    token_ref.assert_reorder_matters(names[:20])
    t = [a for a, _ in names] + [w for w in ssl.synth.gen_corpus(300, seed=5)[0]]
    s = [b for _, b in names] + [w for w in ssl.synth.gen_corpus(100, seed=6)[0]]
    p = Pair(ssl.StringIndex(s), ssl.StringIndex(t), OracleIndex(t))
    try:
        filt = ("levenshtein", 0.9)
        plain, flagged = p.want(0.3, 10, filt, True), p.want(0.3, 10, filt, True, token_sort=True)
        linked = {(p.src[a], p.t.key(int(b))) for a, b in enumerate(flagged[0]) if b != NO_MATCH}
        assert sum(1 for a, b in names if (b, a) in linked) >= 100   # the reordered names link with the flag ...
        assert int((plain[0] != NO_MATCH).sum()) < 20                  # ... and only with it
        check_both_paths(p, 0.3, 10, filt, batches=(0, 37), token_sort=True)
        check_both_paths(p, 0.3, 10, filt, batches=(0,), token_sort=False)
    finally:
        p.dispose()


def wide_words(rng, n):
    alpha = "ABCDEFGHIJKLMNOP" "abcdxyz" "0123456789" " " "éßÖçñ" "日本語中文字" "テキスト" "\U0001F600\U00020000"
    out = set()
    while len(out) < n:
        w = "".join(rng.choice(alpha) for _ in range(rng.randint(4, 16))).strip()
        if len(w) >= 3:
            out.add(w)
    return sorted(out)


def test_link_wide_and_utf8_indexes():
    rng = random.Random(55)
    t = wide_words(rng, 300)
    s = []
    for w in rng.sample(t, 120):
        for _ in range(rng.randint(1, 2)):
            c = list(w)
            c[rng.randrange(len(c))] = rng.choice("QRSTUV日本\U0001F600")
            s.append("".join(c).strip() or "Q")
    s += wide_words(rng, 40)
    og = OracleIndexG(t, 1, None, g=2, wide=True)
    pairs = [Pair(ssl.WideStringIndex(s, gram_size=2), ssl.Utf8StringIndex(t, gram_size=2), og, wide=True),
             Pair(ssl.Utf8StringIndex(s, gram_size=2), ssl.WideStringIndex(t, gram_size=2), og, wide=True)]
    try:
        for p in pairs:
            one, best = p.want(0.4, 5, None, True), p.want(0.4, 5, None, False)
            assert int((one[0] != NO_MATCH).sum()) >= 100 and int((one[0] != best[0]).sum()) >= 5
            assert any(ord(c) > 0xFFFF for k in p.src for c in k)
            check_both_paths(p, 0.4, 5, None, batches=(0, 37))
            check_both_paths(p, 0.4, 5, ("levenshtein", 0.8), batches=(0, 37))
            assert 0 < p.want(0.4, 5, ("levenshtein", 0.8), True)[3] < one[3]
        # a narrow index against a wide one
        narrow = ssl.StringIndex([b"ABCDEF", b"ABCDEG", b"XYZXYZ"])
        with pytest.raises(ValueError):
            narrow.link(pairs[0].t, 0.5)
        with pytest.raises(ValueError):
            pairs[0].s.link(narrow, 0.5)
        L = _native.lib()
        m = (C.c_uint32 * 4)(9, 9, 9, 9)
        L.ngsLastError(1)
        assert L.linkKeys(narrow.handle, pairs[0].t.handle, 0.5, 10, 0, -1.0, 1, 0, m, None, None) == 0
        assert L.ngsLastError(1) == 1 and list(m) == [9] * 4
        narrow.dispose()
    finally:
        for p in pairs:
            p.dispose()


def test_source_keys_are_normalised_by_the_targets_valid_char_set(pair):
    valid = b"ABCDEFGHIJKLM 0123456789"
    s_words, t_words = link_words()
    p = Pair(ssl.StringIndex(s_words), ssl.StringIndex(t_words), OracleIndex(t_words))
    try:
        p.t.set_valid_char(valid)   # the target only: the source keeps the default set
        p.oi.set_valid_char(valid)
        filt = ("levenshtein", 0.5)
        for f in (None, filt):
            assert (p.want(0.3, 5, f, True, valid)[0] != pair.want(0.3, 5, f, True)[0]).sum() >= 10
            check_both_paths(p, 0.3, 5, f, batches=(0, 37), valid=valid)
    finally:
        p.dispose()


def test_the_device_composition_answers_the_models_rows(pair):
    """key_queries_device on S, search_device on T, match_device in rounds: the rows are the model's rows
    and the matching the model's link."""
    thr, limit = 0.5, 10
    rows = pair.rows(thr, limit)
    want = pair.want(thr, limit, None, True)
    ns, nt, ls = pair.ns, pair.nt, min(limit, pair.nt)
    stream = torch.cuda.current_stream().cuda_stream
    total = pair.s.key_query_bytes(0, ns)
    i32 = lambda n, v=-3: torch.full((max(n, 1),), v, dtype=torch.int32, device=DEV)
    buf = torch.zeros(total + 16, dtype=torch.uint8, device=DEV)
    off = torch.zeros(ns + 1, dtype=torch.int64, device=DEV)
    dn, dk, ds = i32(ns), i32(ns * ls), i32(ns * ls)
    ma, mb, bids, matched = i32(ns), i32(nt), torch.zeros(nt, dtype=torch.int64, device=DEV), i32(1)
    torch.cuda.synchronize()
    pair.s.key_queries_device(0, ns, buf.data_ptr(), total, off.data_ptr(), stream)
    pair.t.search_device(buf.data_ptr(), off.data_ptr(), ns, thr, limit, ls, dn.data_ptr(), dk.data_ptr(), ds.data_ptr(),
                         stream)
    gn = dn.cpu().numpy().view(np.uint32)
    gk, gs = dk.cpu().numpy().view(np.uint32).reshape(ns, ls), ds.cpu().numpy().view(np.uint32).reshape(ns, ls)
    for a, (wk, wsc) in enumerate(rows):
        assert gn[a] == len(wk) and np.array_equal(gk[a][:len(wk)], wk) and np.array_equal(gs[a][:len(wk)], wsc), a
    before, first = -1, True
    for _ in range(ns + 1):
        ssl.StringIndex.match_device(dn.data_ptr(), dk.data_ptr(), ds.data_ptr(), ns, ls, 0, ma.data_ptr(), ns,
                                     mb.data_ptr(), nt, bids.data_ptr(), matched.data_ptr(), init=first, stream=stream)
        first = False
        now = int(matched.cpu().numpy()[0])
        if now == before:
            break
        before = now
    assert np.array_equal(ma.cpu().numpy().view(np.uint32), want[0])
    assert before == int((want[0] != NO_MATCH).sum())
