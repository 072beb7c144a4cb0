"""The token sort on the GPU: ngsTokenSortDevice bit for bit against tests/token_ref.py, the similarity
and the re-rank with NGS_SIM_TOKEN_SORT against the model's sim(Q', T'), and score_batch_sim / dedup with
token_sort=True against the oracle's search answers put through the model."""
import ctypes as C
import random

import numpy as np
import pytest

import join_ref
import metric_cases as mc
import metric_ref
import sim_ref
import token_ref
from conftest import fixture_weights, fixture_words, load_fixtures
from metric_cases import DEV, FILL, bits
from oracle_py import OracleIndex, OracleIndexG

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

METRICS = (metric_ref.LEVENSHTEIN, metric_ref.OSA, metric_ref.PARTIAL)
FLAG = token_ref.TOKEN_SORT
NO_TERM = metric_ref.NO_TERM
GUARD_IN, GUARD_OUT = 0xA5, 0x5A


# ---- 1. ngsTokenSortDevice ---------------------------------------------------------------------------
def layout(strings, cs, lead):
    """The strings back to back behind `lead` guard bytes, 64 guard bytes behind them -> (bytes, offsets)."""
    dt = np.uint8 if cs == 1 else np.uint32
    body = b"".join(np.asarray(s, dtype=dt).tobytes() for s in strings)
    offs = np.cumsum([lead] + [len(s) * cs for s in strings], dtype=np.int64)
    return np.frombuffer(bytes([GUARD_IN]) * lead + body + bytes([GUARD_IN]) * 64, dtype=np.uint8).copy(), offs


def device_sort(ix, strings, cs, lead, in_place, qbuf=None):
    """ngsTokenSortDevice over `strings` -> the output strings; the guard bytes around the output are checked."""
    if qbuf is None:
        host, offs = layout(strings, cs, lead)
        raw, off = torch.from_numpy(host).to(DEV), torch.from_numpy(offs).to(DEV)
    else:
        raw, off = qbuf
        offs = off.cpu().numpy()
    out = raw if in_place else torch.full_like(raw, GUARD_OUT)
    s = torch.cuda.Stream()
    mc.ready()
    ix.token_sort_device(raw.data_ptr(), off.data_ptr(), len(strings), out.data_ptr(), s.cuda_stream)
    s.synchronize()
    got = out.cpu().numpy()
    if qbuf is None:
        guard = GUARD_IN if in_place else GUARD_OUT
        assert (got[:offs[0]] == guard).all(), "wrote in front of dOffsets[0]"
        assert (got[offs[-1]:] == guard).all(), "wrote behind dOffsets[n]"
        if not in_place:
            assert np.array_equal(raw.cpu().numpy(), host), "the input was written"
    dt = np.uint8 if cs == 1 else np.uint32
    return [tuple(got[offs[i]:offs[i + 1]].view(dt).tolist()) for i in range(len(strings))]


def check_sort(ix, strings, cs, lead, valid=sim_ref.DEFAULT_VALID, where=""):
    want = [token_ref.token_sort(s, valid, cs == 4) for s in strings]
    assert any(w != tuple(s) for w, s in zip(want, strings))
    for in_place in (False, True):
        got = device_sort(ix, strings, cs, lead, in_place)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{where} in_place={in_place} string {i} ({len(w)} characters): first difference at " \
                           f"{next(j for j in range(len(w)) if g[j] != w[j])}"


def with_tokens(rng, n, alpha, seps=(32,)):
    """A string of n tokens of 1..3 characters: many equal up to case, many prefixes of others."""
    out = []
    for i in range(n):
        if i:
            out += [rng.choice(seps)] * rng.choice((1, 1, 2))
        out += [rng.choice(alpha) for _ in range(rng.randint(1, 3))]
    return out


def sort_cases(rng, alpha, seps, wide):
    body = lambda n: [rng.choice(alpha + [32]) for _ in range(n)]
    cases = [[], [32, 32, 32], list(b",,;"), list(b"*"), list(b" *"),                      # no token
             list(b"single"), list(b"  lead"), list(b"trail \t "), list(b"smith, john"),    # one and two
             list(b"SMITH  JOHN"), list(b"ABC AB A ab"), list(b"ab AB Ab aB"), list(b"b a B A b a")]
    cases += [with_tokens(rng, n, alpha, seps) for n in (63, 64, 65, 100, 129, 700)]
    cases.append(list(b"B A " * 1023 + b"B A"))                                             # 2,048 tokens, 4,095 characters
    sorted_span = [32, 9] + [ord("c")] + body(4094) + [ord("C")] + [32]                     # a span of 4,096: sorted
    kept_span = [32] + [ord("c")] + body(4095) + [ord("C")] + [32, 32]                      # 4,097: unchanged
    far = [32] * 300 + list(b"z y") + [32] * 5000                                           # far longer than its span
    assert token_ref.token_sort(sorted_span, wide=wide) != tuple(sorted_span)
    assert token_ref.token_sort(kept_span, wide=wide) == tuple(kept_span)
    assert token_ref.token_sort(far, wide=wide)[:4] == tuple(b"y z ")
    cases += [sorted_span, kept_span, far]
    if wide:
        cases += [[0x65E5, 0x110000, 0xE9, 32, 65, 0xFFFFFFFF, 0x1F600, 0x80], [0x110000] * 3, [0xE9, 32, 0xE8, 32, 0xE9]]
    else:
        cases += [list(b"b\x80a\xffc"), [0xE9, 32, 65, 0, 66]]
    return cases


@pytest.fixture(scope="module")
def small():
    ix = ssl.StringIndex([b"ALPHA", b"BETA", b"GAMMA DELTA"])
    yield ix
    ix.dispose()


def test_token_sort_narrow(small):
    rng = random.Random(0x81)
    cases = sort_cases(rng, list(b"abAB"), (32, 32, ord(","), 9), False)
    check_sort(small, cases, 1, 7, where="narrow")   # dOffsets[0] = 7: odd byte offsets, shared dwords
    check_sort(small, cases[3:12], 1, 0, where="narrow from 0")


def test_token_sort_custom_valid_set():
    ix = ssl.StringIndex([b"ALPHA", b"BETA", b"GAMMA DELTA"])
    try:
        valid = bytes(c for c in sim_ref.DEFAULT_VALID if c != ord("A")) + b"*"
        ix.set_valid_char(valid)
        rng = random.Random(0x82)
        cases = [list(b"zAa b"), list(b" *"), list(b"*"), list(b"aAa a*"), with_tokens(rng, 70, list(b"abAB*"))]
        check_sort(ix, cases, 1, 3, valid, "a but not A")
        assert device_sort(ix, cases[:2], 1, 3, False) == [tuple(b"a b z"), tuple(b"* ")]
    finally:
        ix.dispose()


def test_token_sort_wide():
    ix = ssl.WideStringIndex(["ALPHA", "BETA", "GAMMA DELTA"])
    try:
        rng = random.Random(0x83)
        cases = sort_cases(rng, [97, 98, 65, 66, 0xE9, 0x65E5], (32, 0x110000, ord("-")), True)
        check_sort(ix, cases, 4, 8, where="wide")
    finally:
        ix.dispose()


def test_token_sort_utf8_handle_behind_the_device_decoder():
    ix = ssl.Utf8StringIndex(["ALPHA", "BETA", "GAMMA DELTA"])
    try:
        rng = random.Random(0x84)
        strings = ["smith, john", "日本 é abc", "b a B A", "", "*", " ".join(rng.choice(["é", "e", "日", "ab", "AB"]) for _ in range(80))]
        q8 = [list(s.encode()) for s in strings]
        raw8, off8 = mc.pack(q8, 1)
        nbytes = sum(map(len, q8))
        out = torch.zeros(4 * nbytes + 16, dtype=torch.uint8, device=DEV)
        out_off = torch.zeros(len(q8) + 1, dtype=torch.int64, device=DEV)
        mc.ready()
        ssl.utf8_decode_device(raw8.data_ptr(), off8.data_ptr(), len(q8), out.data_ptr(), 4 * nbytes, out_off.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        mc.ready()
        got = device_sort(ix, strings, 4, 0, True, qbuf=(out, out_off))
        assert got == [token_ref.token_sort([ord(c) for c in s], wide=True) for s in strings]
    finally:
        ix.dispose()


# ---- 2., 3. the similarity with the flag ---------------------------------------------------------------
NAMES = [b"JOHN SMITH", b"ACME HOLDINGS", b"MARY ANN VON TRAPP", b"GLOBEX   TRADING  CO", b"B  A", b"ZETA"]
LONG = b" ".join(bytes([65 + (i * 7 + j) % 26 for j in range(5)]) for i in range(20))  # 119 characters, 20 words
HUGE = (b"B A " * 1100).strip()                                                           # a term of more than 4,096


class Lib:
    """kind "aliased": rows of three, keys with several terms (kt_off); "unique": one pair per key (key_term)."""

    def __init__(self, kind):
        rng = random.Random(0x85)
        rs = lambda n: bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(n))
        masters = NAMES + [LONG, HUGE] + [rs(rng.randint(4, 9)) + b" " + rs(rng.randint(3, 8)) for _ in range(20)]
        if kind == "aliased":
            words = []
            for w in masters:
                parts = w.split()
                words += [w, b"  ".join(parts[::-1]) if len(parts) > 1 and len(w) < 200 else None, rs(6) + b" X"]
            self.row = 3
        else:
            words, self.row = masters, 1
        self.words = words
        self.ix = ssl.StringIndex(words, self.row)
        dig = (C.c_uint64 * 17)()
        assert _native.lib().ngsIndexDigest(self.ix.handle, dig, 17) == 17
        assert (dig[16] & 1) == (0 if kind == "aliased" else 1), "the corpus does not have the shape this case is about"
        self.nk = self.ix.num_keys()
        self.key_terms = mc.key_term_sets(self.ix, words, self.row)
        self.term_ids = mc.term_table(self.ix)
        terms = set().union(*self.key_terms)
        assert any(len(token_ref.sorted_term(t)) < len(t) for t in terms), "no term with L' < L"
        assert any(len(t) > 4096 and token_ref.sorted_term(t) == t for t in terms)

    def queries(self):
        qs = [b"smith, john", b"holdings acme", b"trapp von ann mary", b"co trading globex", b"a b", b"zeta",
              b"john smyth", b"  SMITH\tJOHN ", b"*", b"", b"   ", b" *"]
        qs.append(b" ".join(LONG.split()[::-1]).lower())           # the long path: m = 119
        qs.append(b" ".join(LONG.split()[3:] + [b"QQQQQ"]))        # ... and not an exact one
        qs.append(b"A B " * 1023 + b"A B")                         # m = 4,095 in 2,048 tokens
        qs.append(b"c" + b"ab " * 1365 + b"C")                     # m = 4,097: not computed
        return [list(q) for q in qs]

    def block(self):
        """Every query against a key id outside the index and every key; the query of 4,095 characters (the
        model pays m x L per pair) against three."""
        qs = self.queries()
        kid = {self.ix.key(k): k for k in range(self.nk)}
        row = [self.nk + 3] + list(range(self.nk))
        keys = [row] * len(qs)
        keys[-2] = [self.nk + 3, kid[LONG], kid[NAMES[0]], kid[HUGE]]
        return qs, [len(r) for r in keys], keys, len(row)


def sorted_buffers(ix, queries):
    """The query batch token-sorted in place on the device, as the flagged device calls expect it."""
    raw, off = mc.pack(queries, 1)
    s = torch.cuda.Stream()
    mc.ready()
    ix.token_sort_device(raw.data_ptr(), off.data_ptr(), len(queries), raw.data_ptr(), s.cuda_stream)
    s.synchronize()
    return raw, off


def expect_flagged(lib, queries, cn, keys, stride, metric):
    want = np.full((len(queries), stride), FILL, dtype=np.uint32)
    want_t = want.copy()
    pairs, cells = [], []
    for i, q in enumerate(queries):
        for r in range(min(cn[i], stride)):
            k = int(keys[i][r])
            pairs.append((tuple(q), lib.key_terms[k] if k < lib.nk else None))
            cells.append((i, r))
    sims, best = token_ref.record_sims(pairs, metric, lib.term_ids)
    for (i, r), b, t in zip(cells, bits(sims), best):
        want[i, r] = b
        want_t[i, r] = NO_TERM if t is None else lib.term_ids[t]
    return want, want_t


def check_flagged(lib, where):
    queries, cn, keys, stride = lib.block()
    qbuf = sorted_buffers(lib.ix, queries)
    star, empty, blanks, bstar = (queries.index(list(q)) for q in (b"*", b"", b"   ", b" *"))
    for metric in METRICS:
        want, want_t = expect_flagged(lib, queries, cn, keys, stride, metric)
        plain, _ = mc.expect_m(queries, cn, keys, stride, lib.key_terms, lib.term_ids, metric)
        assert (want[:4] != plain[:4]).any(axis=1).all(), "the flag changes nothing in the model"
        got, got_t = mc.similarity_m(lib.ix, queries, cn, keys, stride, metric | FLAG, True, qbuf=qbuf)
        mc.check_cells(got, want, f"{where} metric {metric} sims")
        mc.check_cells(got_t, want_t, f"{where} metric {metric} terms")
        alone, none = mc.similarity_m(lib.ix, queries, cn, keys, stride, metric | FLAG, False, qbuf=qbuf)
        assert none is None
        mc.check_cells(alone, want, f"{where} metric {metric} sims without dTerms")
        one, zero, none_ = bits([1.0])[0], bits([0.0])[0], bits([-1.0])[0]
        assert (got[star] == one).all() and (got[empty] == one).all()
        assert (got[blanks, 1:] == zero).all() and (got[bstar, 1:] == zero).all()  # m = 0, no wildcard
        assert (got[-1] == none_).all()
        assert (got[:, 0] == np.where(np.isin(np.arange(len(queries)), (star, empty)), one, none_)).all()
    return queries, cn, keys, stride


def check_plain(lib, where):
    queries, cn, keys, stride = lib.block()
    for metric in METRICS:
        want, want_t = mc.expect_m(queries, cn, keys, stride, lib.key_terms, lib.term_ids, metric)
        got, got_t = mc.similarity_m(lib.ix, queries, cn, keys, stride, metric, True)
        mc.check_cells(got, want, f"{where} metric {metric} sims")
        mc.check_cells(got_t, want_t, f"{where} metric {metric} terms")


def test_similarity_with_the_flag_aliased_index_then_without():
    lib = Lib("aliased")
    try:
        check_flagged(lib, "aliased")
        check_plain(lib, "aliased, unflagged after flagged")
        for t, i in list(lib.term_ids.items())[:10]:  # ngsTerm: the term as indexed
            assert tuple(lib.ix.term(i)) == t
    finally:
        lib.ix.dispose()


def test_similarity_without_the_flag_then_with_it_one_pair_per_key():
    lib = Lib("unique")
    try:
        check_plain(lib, "unique, unflagged first")
        check_flagged(lib, "unique")
        check_plain(lib, "unique, unflagged after flagged")
    finally:
        lib.ix.dispose()


# ---- 4. re-rank -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unique_lib():
    lib = Lib("unique")
    yield lib
    lib.ix.dispose()


@pytest.mark.parametrize("stride", [1, 64, 4096])
def test_rerank_with_the_flag(unique_lib, stride):
    lib = unique_lib
    rng = random.Random(0x86 + stride)
    queries = lib.queries()[:9]
    n = len(queries)
    cn = [min(stride, c) for c in (stride + 3, stride, 40, 0, 1, 64, 65, stride, 7)]
    keys = [[(i + j) % lib.nk if j % 11 else rng.randrange(lib.nk + 2) for j in range(c)] for i, c in enumerate(cn)]
    sc = np.arange(n * stride, dtype=np.float32).reshape(n, stride) * np.float32(0.25) + np.float32(1.0)
    for metric, min_sim in ((metric_ref.LEVENSHTEIN, 0.5), (metric_ref.OSA, 0.3), (metric_ref.PARTIAL, 0.9)):
        want, want_t = expect_flagged(lib, queries, cn, keys, stride, metric)
        raw, off = mc.pack(queries, 1)
        dn, dk = mc.block(cn, keys, stride)
        ds = torch.from_numpy(sc.copy()).to(DEV)
        dv, dt = mc.filled(n * stride), mc.filled(n * stride)
        s = torch.cuda.Stream()
        mc.ready()
        lib.ix.token_sort_device(raw.data_ptr(), off.data_ptr(), n, raw.data_ptr(), s.cuda_stream)
        lib.ix.rerank_device(raw.data_ptr(), off.data_ptr(), n, stride, dn.data_ptr(), dk.data_ptr(), ds.data_ptr(),
                             dv.data_ptr(), min_sim, s.cuda_stream, metric=metric, d_terms=dt.data_ptr(), token_sort=True)
        s.synchronize()
        gn = dn.cpu().numpy().view(np.uint32)
        gk, gs = (d.cpu().numpy().view(np.uint32).reshape(n, stride) for d in (dk, ds))
        gv, gt = (d.cpu().numpy().view(np.uint32) for d in (dv, dt))
        assert (gv[n * stride:] == FILL).all() and (gt[n * stride:] == FILL).all(), "wrote past the block"
        gv, gt = gv[:n * stride].reshape(n, stride), gt[:n * stride].reshape(n, stride)
        dropped = 0
        for i in range(n):
            c = cn[i]
            wk, ws, wv, wt = metric_ref.rerank(list(keys[i][:c]), list(sc[i][:c]), list(want[i][:c].view(np.float32)),
                                               list(want_t[i][:c]), min_sim)
            where = f"stride {stride} metric {metric} query {i}"
            dropped += c - len(wk)
            assert gn[i] == len(wk), f"{where}: keeps {gn[i]}, want {len(wk)}"
            assert gk[i][:len(wk)].tolist() == [int(k) for k in wk], f"{where}: key order"
            assert gs[i][:len(wk)].tolist() == bits(ws).tolist(), f"{where}: scores"
            assert gv[i][:len(wk)].tolist() == bits(wv).tolist(), f"{where}: sims"
            assert gt[i][:len(wk)].tolist() == [int(t) for t in wt], f"{where}: terms"
        assert stride == 1 or dropped > 0, "nothing dropped: the case does not filter"


# ---- 5. score_batch_sim(token_sort=True) ------------------------------------------------------------
def e2e_expected(answers, queries, terms_by_key, term_ids, metric, min_sim, wide=False):
    pairs = [(tuple(sim_ref.units(q, wide)), terms_by_key[tuple(sim_ref.units(k, wide))]) for q, a in zip(queries, answers)
             for k, _ in a]
    sims, best = token_ref.record_sims(pairs, metric, term_ids, sim_ref.DEFAULT_VALID, wide)
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


def test_score_batch_sim_token_sort_on_the_three_classes():
    fx = next(f for f in load_fixtures() if f["name"] == "mixed")
    words, weights, rs = fixture_words(fx), fixture_weights(fx), fx["rowSize"]
    assert rs == 3
    weights = weights if weights is not None else [1.0] * len(words)
    planted = token_ref.reorder_pairs(random.Random(0x87), 12)
    for a, b in planted:  # a key, its reordered alias, and nothing
        words += [a, b, None]
        weights += [1.0, 1.0, 1.0]
    wstr = [None if w is None else w.decode("latin-1") for w in words]
    gi, oi = ssl.StringIndex(words, rs, weights), OracleIndex(words, rs, weights)
    wi, ui = ssl.WideStringIndex(wstr, rs, weights, gram_size=3), ssl.Utf8StringIndex(wstr, rs, weights, gram_size=3)
    og = OracleIndexG(wstr, rs, weights, g=3, wide=True)
    try:
        kt, ktw = sim_ref.key_terms(words, rs, weights), sim_ref.key_terms(wstr, rs, weights, wide=True)
        ids, idw, idu = mc.term_table(gi), mc.term_table(wi, True), mc.term_table(ui, True)
        qs = [c["q"].encode("latin-1") for c in fx["phases"][0]["cases"]][:12]
        qs += [b" ".join(a.split()[::-1]).lower() for a, _ in planted] + [b.replace(b" ", b", ") for _, b in planted[:4]]
        qs += [b"*", b"   "]
        qw = [q.decode("latin-1") for q in qs]
        answers, answers_w = [oi.score(q, 0.3, 8) for q in qs], [og.score(q, 0.3, 8) for q in qw]
        for metric, ms in ((metric_ref.LEVENSHTEIN, 0.5), (metric_ref.OSA, 0.0), (metric_ref.PARTIAL, 0.5)):
            want = e2e_expected(answers, qs, kt, ids, metric, ms)
            got = gi.score_batch_sim(qs, 0.3, 8, ms, metric=metric, with_terms=True, token_sort=True)
            assert e2e_got(got) == want, f"narrow metric {metric}"
            assert [[r[:3] for r in row] for row in got] == gi.score_batch_sim(qs, 0.3, 8, ms, metric=metric | FLAG)
            assert e2e_got(wi.score_batch_sim(qw, 0.3, 8, ms, metric=metric, with_terms=True, token_sort=True), True) == \
                e2e_expected(answers_w, qw, ktw, idw, metric, ms, wide=True), f"wide metric {metric}"
            assert e2e_got(ui.score_batch_sim(qw, 0.3, 8, ms, metric=metric, with_terms=True, token_sort=True), True) == \
                e2e_expected(answers_w, qw, ktw, idu, metric, ms, wide=True), f"utf-8 metric {metric}"
        # the planted keys come back at 1.0 with the flag; without it only where the query is a term as it stands
        flagged = gi.score_batch_sim(qs[12:28], 0.3, 8, 0.0, token_sort=True)
        plain = gi.score_batch_sim(qs[12:28], 0.3, 8, 0.0)
        for (a, _), f, p in zip(planted + planted[:4], flagged, plain):
            assert f[0][0] == a and f[0][2] == 1.0
        for (a, _), p in zip(planted[:4], plain[12:]):  # "WORD, WORD": two blanks after the escape
            assert dict((k, v) for k, _, v in p)[a] < 1.0
    finally:
        for x in (gi, wi, ui):
            x.dispose()


# ---- 6. dedup ---------------------------------------------------------------------------------------
def dedup_want(ix, oi, thr, limit, metric, min_sim, flagged):
    nk = ix.num_keys()
    keys = [ix.key(k) for k in range(nk)]
    gid = {s: k for k, s in enumerate(keys)}
    omap = np.array([gid[oi.key(k)] for k in range(nk)], dtype=np.uint32)
    rows = join_ref.oracle_join(oi, keys, omap, 0, nk, thr, [limit])[limit]
    edges = join_ref.rows_edges(rows)
    term = {k: sim_ref.normalise(s) for k, s in enumerate(keys)}
    record_sims = token_ref.record_sims if flagged else metric_ref.record_sims
    sims, _ = record_sims([(tuple(keys[a]), {term[b]}) for a, b in edges], metric)
    kept = [e for e, v in zip(edges, sims) if not (v < np.float32(min_sim))]
    return join_ref.labels(nk, kept), set(kept), gid


def test_dedup_token_sort_joins_reordered_duplicates():
    rng = random.Random(0x88)
    planted = token_ref.reorder_pairs(rng, 25)
    token_ref.assert_reorder_matters(planted)
    extra = [a for a, _ in token_ref.reorder_pairs(rng, 30)]
    words = [w for p in planted for w in p] + extra
    ix, oi = ssl.StringIndex(words), OracleIndex(words)
    try:
        assert ix.num_keys() == len(set(words)) == len(words)
        want_f, kept_f, gid = dedup_want(ix, oi, 0.3, 10, metric_ref.LEVENSHTEIN, 0.85, True)
        want_p, kept_p, _ = dedup_want(ix, oi, 0.3, 10, metric_ref.LEVENSHTEIN, 0.85, False)
        pairs = [(gid[a], gid[b]) for a, b in planted]
        assert all((a, b) in kept_f and (b, a) in kept_f for a, b in pairs), "the search does not find a planted partner"
        assert all(want_f[a] == want_f[b] for a, b in pairs)
        assert not any(want_p[a] == want_p[b] for a, b in pairs)
        got = ix.dedup(0.3, 10, min_similarity=0.85, token_sort=True)
        assert got == want_f
        assert all(got[a] == got[b] for a, b in pairs)
        assert ix.dedup(0.3, 10, min_similarity=0.85, metric="levenshtein", token_sort=True, batch_keys=17) == want_f
        plain = ix.dedup(0.3, 10, min_similarity=0.85)
        assert plain == want_p and not any(plain[a] == plain[b] for a, b in pairs)
        want_o, _, _ = dedup_want(ix, oi, 0.3, 10, metric_ref.OSA, 0.85, True)
        assert ix.dedup(0.3, 10, min_similarity=0.85, metric=metric_ref.OSA | FLAG) == want_o
    finally:
        ix.dispose()


# ---- 7. save and load ---------------------------------------------------------------------------------
def test_saved_and_loaded_index_gives_the_same_flagged_answers(tmp_path):
    lib = Lib("aliased")
    try:
        qs = [bytes(q) for q in lib.queries()[:12]]
        want = lib.ix.score_batch_sim(qs, 0.2, 10, 0.3, metric="osa", with_terms=True, token_sort=True)
        assert any(r and r[0][2] == 1.0 and r[0][3] != r[0][0] for r in want)
        path = str(tmp_path / "lib.ngs")
        lib.ix.save(path)
        back = ssl.StringIndex.load(path)
        try:
            assert back.score_batch_sim(qs, 0.2, 10, 0.3, metric="osa", with_terms=True, token_sort=True) == want
            queries, cn, keys, stride = lib.block()
            qbuf = sorted_buffers(back, queries)
            want_v, want_t = expect_flagged(lib, queries, cn, keys, stride, metric_ref.PARTIAL)
            got, got_t = mc.similarity_m(back, queries, cn, keys, stride, metric_ref.PARTIAL | FLAG, True, qbuf=qbuf)
            mc.check_cells(got, want_v, "loaded index sims")
            mc.check_cells(got_t, want_t, "loaded index terms")
        finally:
            back.dispose()
    finally:
        lib.ix.dispose()
