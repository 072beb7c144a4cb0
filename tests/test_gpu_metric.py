"""The similarity's metrics and the matched term on the GPU: ngsSimilarityDeviceM / ngsRerankDeviceM on
fabricated result blocks, ngsTerm, scoreBatchSimM* / score_batch_sim(metric=, with_terms=) and
dedup(metric=), against tests/metric_ref.py. Every comparison is exact: fp32 bits, term ids, counts,
key order, labels."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import join_ref
import metric_cases as mc
import metric_ref
import sim_ref
from conftest import fixture_weights, fixture_words, load_fixtures
from metric_cases import DEV, FILL, bits
from oracle_py import OracleIndex, OracleIndexG

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

METRICS = (metric_ref.LEVENSHTEIN, metric_ref.OSA, metric_ref.PARTIAL)
NAMES = {0: "levenshtein", 1: "osa", 2: "partial"}
NO_TERM = metric_ref.NO_TERM


def f32(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def key_ids(ix, wide=False):
    """{key string as a tuple of ints: key id}"""
    return {tuple(sim_ref.units(ix.key(k), wide)): k for k in range(ix.num_keys())}


class Planted:
    """A library around planted queries: for every query its swapped and its embedded variants are keys,
    among random ones. rows(): one result row per (query, count), the query's variants first."""

    def __init__(self, rng, ms, alpha, extra_terms, wide=False, index=None, queries=None):
        self.wide = wide
        self.swaps, self.subs, self.q = [], [], {}
        self.mine = {}  # m -> the words planted for it
        words = []
        for m in ms:
            if queries and m in queries:
                q = tuple(queries[m])
                sw = [(q, tuple(mc.swapped(q, at))) for at in mc.swap_positions(rng, m)] if m >= 2 else []
            else:
                sw = mc.swap_pairs(rng, m, alpha) if m >= 2 else []
                q = sw[0][0] if sw else (rng.choice(alpha),)
            if m > 1000:  # the model pays m x L per pair: the mandated swaps only, in two terms
                sw = [(q, tuple(mc.swapped(q, at))) for at in ([0, 63, 127], [m - 2])]
            sb = [(q, mc.embedded(rng, q, alpha, 1, 9)) for _ in range(1 if m > 1000 else 3)]
            self.q[m] = q
            self.swaps += sw
            self.subs += sb
            self.mine[m] = [t for _, t in sw + sb] + extra_terms(q)
            words += self.mine[m]
        words += [tuple(rng.choice(alpha) for _ in range(rng.randint(1, 70))) for _ in range(60)]
        self.words = words
        as_word = (lambda w: "".join(map(chr, w))) if wide else bytes
        cls = index or (ssl.WideStringIndex if wide else ssl.StringIndex)
        self.ix = cls([as_word(w) for w in words], 1, **({"gram_size": 2} if wide else {}))
        self.kid = key_ids(self.ix, wide)
        self.nk = self.ix.num_keys()
        self.key_terms = mc.key_term_sets(self.ix, [as_word(w) for w in words], wide=wide)
        self.term_ids = mc.term_table(self.ix, wide)

    def raw(self, m):
        """The raw query of length-m Q: lower case where there is one, wrapped in what the trim removes."""
        q = [c + 32 if 65 <= c <= 90 else c for c in self.q[m]]
        return ([32, 9] + q + [32]) if not self.wide else ([32, 0x110000] + q + [9])

    def rows(self, rng, counts):
        queries, cn, keys = [], [], []
        for m in self.q:
            planted = [self.kid[w] for w in self.mine[m] if w in self.kid]
            for n, c in enumerate(counts):
                row = planted[n % 3:] + planted[:n % 3]
                row = (row + [rng.randrange(self.nk) for _ in range(c)])[:c]
                queries.append(self.raw(m))
                cn.append(c)
                keys.append(row)
        return queries, cn, keys

    def check_not_vacuous(self, cn, keys, queries):
        """The anti-vacuity shares on the records of the block itself."""
        in_block = set()
        for q, c, row in zip(queries, cn, keys):
            nq = sim_ref.normalise(q, sim_ref.DEFAULT_VALID, self.wide)
            for k in row[:c]:
                in_block |= {(nq, t) for t in self.key_terms[k]} if k < self.nk else set()
        sw = [p for p in self.swaps if p in in_block]
        sb = [p for p in self.subs if p in in_block]
        assert len(sw) >= len(self.q) and len(sb) >= len(self.q) - 1, (len(sw), len(sb))
        mc.assert_not_vacuous(sw, sb)


def run_all_metrics(lib, queries, cn, keys, stride, cs, where, qbuf=None):
    for metric in METRICS:
        want, want_t = mc.expect_m(queries, cn, keys, stride, lib.key_terms, lib.term_ids, metric, wide=lib.wide)
        got, got_t = mc.similarity_m(lib.ix, queries, cn, keys, stride, NAMES[metric], True, cs, qbuf)
        mc.check_cells(got, want, f"{where} {NAMES[metric]} sims")
        mc.check_cells(got_t, want_t, f"{where} {NAMES[metric]} terms")
        alone, none = mc.similarity_m(lib.ix, queries, cn, keys, stride, metric, False, cs, qbuf)
        assert none is None
        mc.check_cells(alone, want, f"{where} {NAMES[metric]} sims without dTerms")


# ---- the short path ---------------------------------------------------------------------------
SHORT_M = (1, 2, 3, 31, 32, 33, 63, 64)
COUNTS = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def narrow():
    rng = random.Random(0x71)
    lib = Planted(rng, SHORT_M, mc.ALPHA36, lambda q: [])
    yield lib
    lib.ix.dispose()


def test_short_path_narrow(narrow):
    lib = narrow
    rng = random.Random(0x72)
    queries, cn, keys = lib.rows(rng, COUNTS)
    for q, m in zip(queries[::len(COUNTS)], SHORT_M):
        assert len(sim_ref.normalise(q)) == m
    lib.check_not_vacuous(cn, keys, queries)
    # nothing left after the trim, wildcards, key ids outside the index
    queries += [list(b" \t# "), list(b"*"), [], lib.raw(8) if 8 in lib.q else lib.raw(3)]
    cn += [65, 64, 3, 6]
    keys += [[rng.randrange(lib.nk) for _ in range(65)], [rng.randrange(lib.nk) for _ in range(64)], [0, lib.nk, 1],
             [0, lib.nk, 0xFFFFFFFF, lib.nk - 1, lib.nk + 1, 2]]
    run_all_metrics(lib, queries, cn, keys, 130, 1, "short narrow")
    for metric in METRICS:
        _, want_t = mc.expect_m(queries, cn, keys, 130, lib.key_terms, lib.term_ids, metric)
        assert (want_t[-3][:64] == NO_TERM).all() and want_t[-1][1] == want_t[-1][2] == NO_TERM != want_t[-1][0]


def wide_chars():
    slot = lambda c: ((c * 0x9E3779B1) & 0xFFFFFFFF) >> 25
    seen = {}
    for c in range(0x4E00, 0x5000):
        if slot(c) in seen:
            return seen[slot(c)], c
        seen[slot(c)] = c
    raise AssertionError("no collision")


def wide_lib(index=None):
    rng = random.Random(0x73)
    c1, c2 = wide_chars()  # two characters of one home slot in the match-mask table
    alpha = [ord(c) for c in "ABCD09"] + [0xE9, 0xFF, 0x100, 0x65E5, 0x672C, c1, c2, 0x1F600, 0x10FFFF]
    distinct = [0x3041 + i for i in range(62)] + [c1, c2]  # 64 distinct characters: the table's full load
    return Planted(rng, (2, 5, 33, 64), alpha, lambda q: [], wide=True, index=index,
                   queries={64: distinct, 5: [c1, c2, c1, ord("A"), c2]})


def test_short_path_wide():
    lib = wide_lib()
    try:
        rng = random.Random(0x74)
        queries, cn, keys = lib.rows(rng, (1, 63, 64, 65))
        lib.check_not_vacuous(cn, keys, queries)
        run_all_metrics(lib, queries, cn, keys, 65, 4, "short wide")
    finally:
        lib.ix.dispose()


def test_short_path_utf8_handle_behind_the_device_decoder():
    lib = wide_lib(index=ssl.Utf8StringIndex)
    try:
        rng = random.Random(0x75)
        queries, cn, keys = lib.rows(rng, (1, 64, 65))
        enc = lambda q: b"".join(chr(c).encode() if c <= 0x10FFFF else bytes([0xFF]) for c in q)  # 0xFF: an invalid byte
        q8 = [enc(q) for q in queries]
        units = [[c if c <= 0x10FFFF else 0x110000 + 0xFF for c in q] for q in queries]  # what the decoder makes of it
        raw8, off8 = mc.pack([list(q) for q in q8], 1)
        nbytes = sum(len(q) for q in q8)
        out = torch.zeros(4 * nbytes + 16, dtype=torch.uint8, device=DEV)
        out_off = torch.zeros(len(q8) + 1, dtype=torch.int64, device=DEV)
        mc.ready()
        ssl.utf8_decode_device(raw8.data_ptr(), off8.data_ptr(), len(q8), out.data_ptr(), 4 * nbytes, out_off.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        mc.ready()
        run_all_metrics(lib, units, cn, keys, 65, 4, "utf-8 handle", qbuf=(out, out_off))
    finally:
        lib.ix.dispose()


# ---- the long path ----------------------------------------------------------------------------
LONG_M = (65, 127, 128, 129, 200, 4096)


def long_case(wide):
    rng = random.Random(0x76 + wide)
    alpha = ([ord(c) for c in "ABCDEFGH"] + [0xE9, 0x65E5, 0x1F600, 0x100]) if wide else mc.ALPHA36
    rs = lambda n: tuple(rng.choice(alpha) for _ in range(n))

    def extra(q):  # L in {1, 63, 64, 65, m, m + 70}: random ones, the query's own prefixes, an embedded one
        m = len(q)
        inner = list(q)
        inner[m // 2] = next(c for c in alpha if c != inner[m // 2])
        return [rs(1), rs(63), rs(64), rs(65), q[:63], q[:64], q[1:66], tuple(rs(30) + tuple(inner) + rs(40))] + \
            ([q] if m < 1000 else [])

    lib = Planted(rng, LONG_M, alpha, extra, wide=wide)
    try:
        for m in LONG_M:
            assert {len(t) for t in lib.mine[m]} >= {1, 63, 64, 65, m, m + 70}
            diffs = [{i for i in range(m) if q[i] != t[i]} for q, t in lib.swaps if len(q) == m]
            for rows in ({0, 1}, {m - 2, m - 1}, {63, 64}) + (({127, 128},) if m > 128 else ()):
                assert any(rows <= d for d in diffs), (m, rows)
            lib.subs += [(lib.q[m], t) for t in lib.mine[m] if len(t) == m + 70]
        queries, cn, keys = [], [], []
        for m in LONG_M:
            row = [lib.kid[w] for w in lib.mine[m]] + [rng.randrange(lib.nk) for _ in range(3)] + [lib.nk + 5]
            queries.append(lib.raw(m))
            cn.append(len(row))
            keys.append(row)
        lib.check_not_vacuous(cn, keys, queries)
        # one character too many: not computed, whatever the metric
        over = [32] + list(lib.q[4096]) + [ord("A")] + [32]
        assert len(sim_ref.normalise(over, sim_ref.DEFAULT_VALID, wide)) == 4097
        queries.append(over)
        cn.append(5)
        keys.append(keys[-1][:5])
        stride = max(cn)
        run_all_metrics(lib, queries, cn, keys, stride, 4 if wide else 1, f"long wide={wide}")
        for metric in METRICS:
            got, got_t = mc.similarity_m(lib.ix, queries[-1:], [5], keys[-1:], 5, metric, True, 4 if wide else 1)
            assert (got == bits([-1.0])[0]).all() and (got_t == NO_TERM).all()
    finally:
        lib.ix.dispose()


def test_long_path_narrow():
    long_case(False)


def test_long_path_wide():
    long_case(True)


# ---- metric 0 through the M entry points ------------------------------------------------------------
def rerank_run(ix, queries, cn, keys, stride, min_sim, metric=None, with_terms=False):
    """ngsRerankDevice(M) on a fabricated block (scores: distinct values) -> counts, keys, score bits, sim
    bits, term ids (or None), each checked for writes past the block."""
    n = len(queries)
    raw, off = mc.pack(queries, 1)
    dn, dk = mc.block(cn, keys, stride)
    sc = np.arange(n * stride, dtype=np.float32).reshape(n, stride) * np.float32(0.25) + np.float32(1.0)
    ds = torch.from_numpy(sc.copy()).to(DEV)
    dv, dt = mc.filled(n * stride), mc.filled(n * stride) if with_terms else None
    s = torch.cuda.Stream()
    mc.ready()
    ix.rerank_device(raw.data_ptr(), off.data_ptr(), n, stride, dn.data_ptr(), dk.data_ptr(), ds.data_ptr(),
                     dv.data_ptr(), min_sim, s.cuda_stream, metric=metric, d_terms=dt.data_ptr() if with_terms else 0)
    s.synchronize()
    out = [dn.cpu().numpy().view(np.uint32), dk.cpu().numpy().view(np.uint32).reshape(n, stride),
           ds.cpu().numpy().view(np.uint32).reshape(n, stride)]
    for d in (dv, dt):
        if d is None:
            out.append(None)
            continue
        a = d.cpu().numpy().view(np.uint32)
        assert (a[n * stride:] == FILL).all(), "wrote past the block"
        out.append(a[:n * stride].reshape(n, stride))
    return out, sc


def test_metric_0_equals_the_entry_points_without_a_metric(narrow):
    lib = narrow
    rng = random.Random(0x77)
    queries, cn, keys = lib.rows(rng, (1, 64, 65, 130))
    stride = 130
    n = len(queries)
    raw, off = mc.pack(queries, 1)
    dn, dk = mc.block(cn, keys, stride)
    dv = mc.filled(n * stride)
    mc.ready()
    lib.ix.similarity_device(raw.data_ptr(), off.data_ptr(), n, stride, dn.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    mc.ready()
    old = dv.cpu().numpy().view(np.uint32)[:n * stride].reshape(n, stride)
    new, _ = mc.similarity_m(lib.ix, queries, cn, keys, stride, 0, False)
    assert np.array_equal(old, new)
    new, _ = mc.similarity_m(lib.ix, queries, cn, keys, stride, "levenshtein", True)
    assert np.array_equal(old, new)
    for ms in (0.0, 0.6):
        a, _ = rerank_run(lib.ix, queries, cn, keys, stride, ms)
        b, _ = rerank_run(lib.ix, queries, cn, keys, stride, ms, metric=0)
        c, _ = rerank_run(lib.ix, queries, cn, keys, stride, ms, metric=0, with_terms=True)
        assert 0 < a[0].sum() < sum(cn) or ms == 0.0
        for i in range(n):
            k = int(a[0][i])
            assert k == b[0][i] == c[0][i], f"min {ms}: query {i} counts"
            for x in (1, 2, 3):
                assert np.array_equal(a[x][i][:k], b[x][i][:k]) and np.array_equal(a[x][i][:k], c[x][i][:k]), \
                    f"min {ms}: query {i} array {x}"


# ---- the matched term -----------------------------------------------------------------------------
ALIAS_QUERIES = [b"proxima", b"rigil kent", b"alpha centauri", b"visible alias", b"hidden master", b"shared term",
                 b"beta orionis", b"negative", b"only alias", b"zzz", b"solo", b"*", b"tie abcdz", b"twin 1x"]


def alias_check(words, weights, unique):
    ix = ssl.StringIndex(words, 3, weights)
    try:
        dig = (C.c_uint64 * 17)()
        assert _native.lib().ngsIndexDigest(ix.handle, dig, 17) == 17
        assert (dig[16] & 1) == (1 if unique else 0), "the corpus does not have the shape this case is about"
        key_terms = mc.key_term_sets(ix, words, 3, weights)
        term_ids = mc.term_table(ix)
        assert set(term_ids) == set().union(*key_terms), "ngsTerm's terms are not the model's"
        assert sorted(term_ids.values()) == list(range(ix.size()))
        L = _native.lib()
        for t, i in term_ids.items():
            assert L.ngsTerm(ix.handle, i, None, 0) == len(t)
            buf = (C.c_uint8 * 8)(*([0xAA] * 8))
            assert L.ngsTerm(ix.handle, i, buf, 3) == len(t)  # a short buffer: the length, and what fits
            assert bytes(buf[:3]) == bytes(t[:3]) + b"\xaa" * (3 - min(3, len(t))) and bytes(buf[3:]) == b"\xaa" * 5
        assert L.ngsTerm(ix.handle, ix.size(), None, 0) == -3
        with pytest.raises(IndexError):
            ix.term(ix.size())
        nk = ix.num_keys()
        qs = [list(q) for q in ALIAS_QUERIES]
        cn = [nk + 2] * len(qs)
        keys = [list(range(nk)) + [nk, 0xFFFFFFFF] for _ in qs]
        by_id = {i: t for t, i in term_ids.items()}
        out = {}
        for metric in METRICS:
            want, want_t = mc.expect_m(qs, cn, keys, nk + 2, key_terms, term_ids, metric)
            got, got_t = mc.similarity_m(ix, qs, cn, keys, nk + 2, metric, True)
            mc.check_cells(got, want, f"aliases unique={unique} {NAMES[metric]} sims")
            mc.check_cells(got_t, want_t, f"aliases unique={unique} {NAMES[metric]} terms")
            # said again without the model's choice of term: the term belongs to the key and has the record's similarity
            for i, q in enumerate(qs):
                for k in range(nk):
                    if got_t[i][k] == NO_TERM:
                        continue
                    t = by_id[int(got_t[i][k])]
                    assert t in key_terms[k]
                    one, _ = metric_ref.record_sims([(tuple(q), {t})], metric)
                    assert bits(one)[0] == got[i][k]
            star = ALIAS_QUERIES.index(b"*")
            assert (got_t[star] == NO_TERM).all() and (got_t[:, nk:] == NO_TERM).all()
            out[metric] = (got, got_t)
        return ix.num_keys(), out, {ix.key(k): k for k in range(nk)}, term_ids
    finally:
        ix.dispose()


def test_matched_term_keys_with_several_terms():
    words = [b"ALPHA CENTAURI", b"PROXIMA", b"RIGIL KENT",
             b"HIDDEN MASTER", b"VISIBLE ALIAS", None,          # master weight 0: an alias-only key
             b"BETA ORIONIS", b"SHARED TERM", b"RIGEL",
             b"GAMMA CRUCIS", b"SHARED TERM", b"NEGATIVE",      # one term under two keys; negative weights
             b"SOLO", None, None,
             b"TIE MASTER", b"TIE ABCDY", b"TIE ABCDX",         # planted ties: two aliases at one similarity
             b"TWIN", b"TWIN X1", b"TWIN 1X"]                   # ... and one a swap away under OSA only
    weights = [1.0, 0.5, 2.0, 0.0, 1.0, 1.0, 1.0, 1.0, -1.0, -0.5, 0.25, -2.0, 1.0, 1.0, 1.0,
               1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    nk, out, kid, term_ids = alias_check(words, weights, unique=False)
    assert nk == 7
    tid = lambda s: term_ids[tuple(s)]
    for metric in METRICS:
        got, got_t = out[metric]
        row = lambda q: got_t[ALIAS_QUERIES.index(q)]
        assert row(b"proxima")[kid[b"ALPHA CENTAURI"]] == tid(b"PROXIMA")  # the alias, not the master
        assert row(b"visible alias")[kid[b"HIDDEN MASTER"]] == tid(b"VISIBLE ALIAS")
        assert row(b"shared term")[kid[b"BETA ORIONIS"]] == row(b"shared term")[kid[b"GAMMA CRUCIS"]] == tid(b"SHARED TERM")
        # "TIE ABCDZ" is one substitution from both aliases: the smaller term id, whatever their order in the key
        assert row(b"tie abcdz")[kid[b"TIE MASTER"]] == min(tid(b"TIE ABCDY"), tid(b"TIE ABCDX"))
    # "TWIN 1X": equal to one alias, a swap from the other
    q = ALIAS_QUERIES.index(b"twin 1x")
    assert out[metric_ref.OSA][1][q][kid[b"TWIN"]] == tid(b"TWIN 1X")
    assert f32(out[metric_ref.OSA][0][q][kid[b"TWIN"]]) == 1.0


def test_matched_term_keys_with_one_pair_each():
    words = [b"ALPHA CENTAURI", None, None,
             b"HIDDEN MASTER", b"ONLY ALIAS", None,              # master weight 0: its one pair is the alias
             b"BETA ORIONIS", b"SHARED TERM", None,              # one term under two keys, each key's only pair
             b"GAMMA CRUCIS", b"PROXIMA", b"SHARED TERM",
             b"SOLO", b"RIGIL KENT", b"NEGATIVE"]
    weights = [1.0, 1.0, 1.0, 0.0, -1.5, 1.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.5, 0.0, 0.0, -2.0]
    nk, out, kid, term_ids = alias_check(words, weights, unique=True)
    assert nk == 5
    tid = lambda s: term_ids[tuple(s)]
    for metric in METRICS:
        got, got_t = out[metric]
        row = lambda q: got_t[ALIAS_QUERIES.index(q)]
        assert row(b"only alias")[kid[b"HIDDEN MASTER"]] == tid(b"ONLY ALIAS")
        assert row(b"shared term")[kid[b"BETA ORIONIS"]] == row(b"shared term")[kid[b"GAMMA CRUCIS"]] == tid(b"SHARED TERM")
        assert row(b"zzz")[kid[b"SOLO"]] == tid(b"NEGATIVE")


# ---- re-rank with terms ------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 64, 65, 100, 4096])
def test_rerank_with_terms(narrow, stride):
    lib = narrow
    rng = random.Random(0x78 + stride)
    ms = [m for m in SHORT_M if m >= 2]
    queries = [lib.raw(ms[i % len(ms)]) for i in range(6)] + [list(b"*")]
    cn = [stride + 5, stride, max(1, stride // 2), 0, 1, min(stride, 70), stride]  # the first: above the stride
    keys = []
    for i, c in enumerate(cn):
        c = min(c, stride)
        planted = [lib.kid[w] for w in lib.mine[ms[i % len(ms)]] if w in lib.kid]
        row = [planted[j % len(planted)] if j % 3 == 0 else rng.randrange(lib.nk) for j in range(c)]
        for j in range(5, c, 37):
            row[j] = lib.nk + j  # outside the index: sim -1, no term
        keys.append(row)
    for metric, min_sim in ((metric_ref.OSA, 0.3), (metric_ref.PARTIAL, 0.5), (metric_ref.LEVENSHTEIN, -1.0)):
        want, want_t = mc.expect_m(queries, cn, keys, stride, lib.key_terms, lib.term_ids, metric)
        (gn, gk, gs, gv, gt), sc = rerank_run(lib.ix, queries, cn, keys, stride, min_sim, NAMES[metric], True)
        dropped = 0
        for i in range(len(queries)):
            c = min(cn[i], stride)
            wk, ws, wv, wt = metric_ref.rerank(list(keys[i][:c]), list(sc[i][:c]), list(want[i][:c].view(np.float32)),
                                               list(want_t[i][:c]), min_sim)
            where = f"stride {stride} {NAMES[metric]} query {i}"
            dropped += c - len(wk)
            assert gn[i] == len(wk), f"{where}: keeps {gn[i]}, want {len(wk)}"
            assert gk[i][:len(wk)].tolist() == [int(k) for k in wk], f"{where}: key order"
            assert gs[i][:len(wk)].tolist() == bits(ws).tolist(), f"{where}: scores do not travel with their keys"
            assert gv[i][:len(wk)].tolist() == bits(wv).tolist(), f"{where}: sims"
            assert gt[i][:len(wk)].tolist() == [int(t) for t in wt], f"{where}: terms do not travel with their keys"
        assert min_sim < 0 or stride == 1 or dropped > 0, "nothing dropped: the case does not filter"
        # without dTerms: the same three arrays
        (bn, bk, bs, bv, _), _ = rerank_run(lib.ix, queries, cn, keys, stride, min_sim, metric, False)
        for i in range(len(queries)):
            k = int(gn[i])
            assert bn[i] == k and np.array_equal(bk[i][:k], gk[i][:k]) and np.array_equal(bs[i][:k], gs[i][:k]) and \
                np.array_equal(bv[i][:k], gv[i][:k])


# ---- end to end ---------------------------------------------------------------------------------
def e2e_expected(answers, queries, terms_by_key, term_ids, valid, metric, min_sim, wide=False):
    """Oracle answers [(key, score)] per query -> [(key, score bits, sim bits, term)] after the similarity and the re-rank."""
    pairs = [(tuple(sim_ref.units(q, wide)), terms_by_key[tuple(sim_ref.units(k, wide))]) for q, a in zip(queries, answers)
             for k, _ in a]
    sims, best = metric_ref.record_sims(pairs, metric, term_ids, valid, wide)
    out, o = [], 0
    for a in answers:
        ks, ss, vs, ts = metric_ref.rerank([k for k, _ in a], [s for _, s in a], list(sims[o:o + len(a)]),
                                           best[o:o + len(a)], min_sim)
        out.append([(k, int(bits([s])[0]), int(bits([v])[0]), t) for k, s, v, t in zip(ks, ss, vs, ts)])
        o += len(a)
    return out


def e2e_got(rows, wide=False):
    return [[(k, int(bits([s])[0]), int(bits([v])[0]), None if t is None else tuple(sim_ref.units(t, wide)))
             for k, s, v, t in r] for r in rows]


@pytest.mark.parametrize("name", ["synth_c1", "mixed"])
def test_end_to_end_on_golden_corpora(name):
    fx = next(f for f in load_fixtures() if f["name"] == name)
    words, weights, rs = fixture_words(fx), fixture_weights(fx), fx["rowSize"]
    wstr = [None if w is None else w.decode("latin-1") for w in words]
    gi, oi = ssl.StringIndex(words, rs, weights), OracleIndex(words, rs, weights)
    wi, ui = ssl.WideStringIndex(wstr, rs, weights, gram_size=3), ssl.Utf8StringIndex(wstr, rs, weights, gram_size=3)
    og = OracleIndexG(wstr, rs, weights, g=3, wide=True)
    try:
        kt = sim_ref.key_terms(words, rs, weights)
        ktw = sim_ref.key_terms(wstr, rs, weights, wide=True)
        ids, idw, idu = mc.term_table(gi), mc.term_table(wi, True), mc.term_table(ui, True)
        valid = sim_ref.DEFAULT_VALID
        for ph in fx["phases"]:
            if ph["validChar"] is not None:
                valid = ph["validChar"].encode("latin-1")
                for x in (gi, oi, wi, ui, og):
                    x.set_valid_char(valid)
            groups = {}
            for c in ph["cases"]:
                groups.setdefault((c["thr"], c["limit"]), []).append(c["q"].encode("latin-1"))
            for (tb, limit), qs in groups.items():
                thr = f32(tb)
                if min(limit or 2 ** 31, gi.num_keys()) > sim_ref.RERANK_MAX_STRIDE:
                    continue
                answers = [oi.score(q, thr, limit) for q in qs]
                qw = [q.decode("latin-1") for q in qs]
                answers_w = [og.score(q, thr, limit) for q in qw]
                for metric, ms in ((metric_ref.OSA, 0.4), (metric_ref.PARTIAL, 0.0), (metric_ref.LEVENSHTEIN, 0.4)):
                    where = f"{name} thr={thr} limit={limit} {NAMES[metric]} min={ms}"
                    want = e2e_expected(answers, qs, kt, ids, valid, metric, ms)
                    got = gi.score_batch_sim(qs, thr, limit, ms, metric=NAMES[metric], with_terms=True)
                    assert e2e_got(got) == want, where
                    plain = gi.score_batch_sim(qs, thr, limit, ms, metric=metric)
                    assert [[r[:3] for r in row] for row in got] == plain, where + " (without terms)"
                    assert e2e_got(wi.score_batch_sim(qw, thr, limit, ms, metric=metric, with_terms=True), True) == \
                        e2e_expected(answers_w, qw, ktw, idw, valid, metric, ms, wide=True), where + " (wide)"
                    assert e2e_got(ui.score_batch_sim(qw, thr, limit, ms, metric=metric, with_terms=True), True) == \
                        e2e_expected(answers_w, qw, ktw, idu, valid, metric, ms, wide=True), where + " (utf-8)"
    finally:
        for x in (gi, wi, ui):
            x.dispose()


def test_end_to_end_small_wide_corpus_gram_size_2():
    rng = random.Random(0x79)
    alpha = "ABCDE日本語é "
    base = ["".join(rng.choice(alpha) for _ in range(rng.randint(2, 14))).strip() or "AB" for _ in range(150)]
    words = []
    for w in base:  # a key, and an alias one adjacent swap away
        p = rng.randrange(len(w) - 1) if len(w) > 1 else 0
        words += [w, w[:p] + w[p + 1:p + 2] + w[p:p + 1] + w[p + 2:]]
    wi, ui = ssl.WideStringIndex(words, 2, gram_size=2), ssl.Utf8StringIndex(words, 2, gram_size=2)
    og = OracleIndexG(words, 2, None, g=2, wide=True)
    try:
        kt = sim_ref.key_terms(words, 2, None, wide=True)
        qs = [w.lower() for w in rng.sample(base, 25)] + [w[1:] + "x" for w in rng.sample(base, 10)] + ["*", "日本"]
        answers = [og.score(q, 0.2, 12) for q in qs]
        for ix in (wi, ui):
            ids = mc.term_table(ix, True)
            for metric, ms in ((metric_ref.OSA, 0.5), (metric_ref.PARTIAL, 0.6), (metric_ref.LEVENSHTEIN, 0.0)):
                want = e2e_expected(answers, qs, kt, ids, sim_ref.DEFAULT_VALID, metric, ms, wide=True)
                got = ix.score_batch_sim(qs, 0.2, 12, ms, metric=NAMES[metric], with_terms=True)
                assert e2e_got(got, True) == want, f"{type(ix).__name__} {NAMES[metric]}"
                assert any(t is not None and tuple(map(ord, k)) != t for row in got for k, _, _, t in row)
    finally:
        wi.dispose()
        ui.dispose()


def test_unknown_metric_end_to_end(narrow):
    L = _native.lib()
    qs = (C.c_char_p * 2)(b"abc", b"*")
    counts = (C.c_uint32 * 2)(9, 9)
    res = C.POINTER(C.POINTER(C.c_char))()
    sc, sv, tv = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
    L.ngsLastError(1)
    assert L.scoreBatchSimM(narrow.ix.handle, qs, 2, 0.0, 10, 3, 0.0, counts, C.byref(res), C.byref(sc), C.byref(sv),
                            C.byref(tv)) == 0
    assert L.ngsLastError(1) == 1 and list(counts) == [0, 0] and not res and not sc and not sv and not tv
    with pytest.raises(ValueError):
        narrow.ix.score_batch_sim([b"abc"], metric="jaro")


# ---- dedup ----------------------------------------------------------------------------------------
def dedup_want(ix, oi, thr, limit, metric, min_sim):
    """(labels, kept edges, edges): join_ref's union-find over the oracle's join edges the model keeps."""
    nk = ix.num_keys()
    keys = [ix.key(k) for k in range(nk)]
    gid = {s: k for k, s in enumerate(keys)}
    omap = np.array([gid[oi.key(k)] for k in range(nk)], dtype=np.uint32)
    rows = join_ref.oracle_join(oi, keys, omap, 0, nk, thr, [limit])[limit]
    edges = join_ref.rows_edges(rows)
    term = {k: sim_ref.normalise(s) for k, s in enumerate(keys)}
    sims, _ = metric_ref.record_sims([(tuple(keys[a]), {term[b]}) for a, b in edges], metric)
    kept = [e for e, v in zip(edges, sims) if not (v < np.float32(min_sim))]
    return join_ref.labels(nk, kept), set(kept), edges, gid


def test_dedup_by_metric_joins_keys_one_swap_apart():
    rng = random.Random(0x7A)
    base = [bytes(mc.no_equal_neighbours(rng, 10, b"ABCDEFGHIJKLMNOPQRSTUVWXYZ")) for _ in range(300)]
    partners = {}
    for w in rng.sample(base, 120):
        p = rng.randrange(9)
        partners[w] = w[:p] + w[p + 1:p + 2] + w[p:p + 1] + w[p + 2:]
    words = base + list(partners.values())
    ix, oi = ssl.StringIndex(words), OracleIndex(words)
    try:
        assert ix.num_keys() == len(set(words)) == len(words)
        want_o, kept_o, edges, gid = dedup_want(ix, oi, 0.3, 10, metric_ref.OSA, 0.85)
        want_l, kept_l, _, _ = dedup_want(ix, oi, 0.3, 10, metric_ref.LEVENSHTEIN, 0.85)
        pairs = [(gid[a], gid[b]) for a, b in partners.items()]
        # by the model: one swap is 0.9 under OSA and 0.8 under Levenshtein
        assert all((a, b) in kept_o and (b, a) in kept_o for a, b in pairs), "the search does not find a planted partner"
        assert all(want_o[a] == want_o[b] for a, b in pairs)
        assert not any((a, b) in kept_l or (b, a) in kept_l for a, b in pairs)
        joined_l = [(a, b) for a, b in pairs if want_l[a] == want_l[b]]  # only through another edge, if at all
        assert len(joined_l) < len(pairs) // 4
        assert ix.dedup(0.3, 10, min_similarity=0.85, metric="osa") == want_o
        assert ix.dedup(0.3, 10, min_similarity=0.85, metric="levenshtein") == want_l
        assert ix.dedup(0.3, 10, min_similarity=0.85) == want_l
        assert ix.dedup(0.3, 10, min_similarity=0.85, metric=1, batch_keys=77) == want_o
    finally:
        ix.dispose()


def test_dedup_partial_joins_keys_that_contain_other_keys():
    rng = random.Random(0x7B)
    rs = lambda n: bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(n))
    base = [rs(7) for _ in range(120)]
    words = list(base)
    holders = {}
    for w in rng.sample(base, 50):
        holders[w] = w + b" " + rs(rng.randint(4, 7))
        words.append(holders[w])
    ix, oi = ssl.StringIndex(words), OracleIndex(words)
    try:
        want_p, kept_p, edges, gid = dedup_want(ix, oi, 0.3, 10, metric_ref.PARTIAL, 0.85)
        want_l, kept_l, _, _ = dedup_want(ix, oi, 0.3, 10, metric_ref.LEVENSHTEIN, 0.85)
        pairs = [(gid[a], gid[b]) for a, b in holders.items()]
        # directional: the row of the short key keeps the record, the row of the long one need not
        assert all((a, b) in kept_p for a, b in pairs) and not all((b, a) in kept_p for a, b in pairs)
        assert all(want_p[a] == want_p[b] for a, b in pairs) and not any(want_l[a] == want_l[b] for a, b in pairs)
        assert ix.dedup(0.3, 10, min_similarity=0.85, metric="partial") == want_p
    finally:
        ix.dispose()
