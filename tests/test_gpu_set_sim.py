"""The later stages over an index set on the GPU: ngsSetSimilarityDeviceM on planted records against the
per-member model (tests/metric_ref.py, tests/token_ref.py with each member's term table), and
scoreBatchSetSimM*, selfJoinSet, dedupKeysSet and the device forms against one index over the same rows.
Every comparison is exact: fp32 bits, term ids, counts, key strings and order, clusters."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import join_ref
import metric_cases as mc
import metric_ref
import set_corpus
import sim_ref
import token_ref
from metric_cases import DEV, FILL, bits

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

METRICS = (metric_ref.LEVENSHTEIN, metric_ref.OSA, metric_ref.PARTIAL)
NO_TERM = metric_ref.NO_TERM
FLAG = token_ref.TOKEN_SORT
STRIDE = 129
COUNTS = (1, 63, 64, 65, 129)
LENGTHS = (1, 63, 64, 65, 128, 129)


def unique_flag(ix):
    dig = (C.c_uint64 * 17)()
    assert _native.lib().ngsIndexDigest(ix.handle, dig, 17) == 17
    return dig[16] & 1


class Member:
    """One index with the model's view of it: every key's terms and the term ids."""

    def __init__(self, words, row, wide, unique):
        as_word = (lambda w: None if w is None else "".join(map(chr, w))) if wide else \
            (lambda w: None if w is None else bytes(w))
        strings = [as_word(w) for w in words]
        self.ix = (ssl.WideStringIndex(strings, row, gram_size=2) if wide else ssl.StringIndex(strings, row))
        assert unique_flag(self.ix) == (1 if unique else 0), "the member does not have the storage form this case needs"
        self.nk = self.ix.num_keys()
        self.key_terms = mc.key_term_sets(self.ix, strings, row, wide=wide)
        self.term_ids = mc.term_table(self.ix, wide)
        self.kid = {tuple(sim_ref.units(self.ix.key(k), wide)): k for k in range(self.nk)}


class PlantedSet:
    """16 small members around planted queries: the query's swapped and embedded variants are keys, dealt
    to the members in turn, among random ones. Even members hold rows of (key, alias, alias) and list every
    key's terms (kt_off); odd ones hold one pair per key (the key_term map)."""

    def __init__(self, wide):
        rng = random.Random(0x91 + wide)
        self.wide = wide
        alpha = ([ord(c) for c in "ABCDEFGH"] + [0xE9, 0x65E5, 0x1F600, 0x100]) if wide else mc.ALPHA36
        rs = lambda n: tuple(rng.choice(alpha) for _ in range(n))
        self.q, swaps, subs = {}, [], []
        for m in LENGTHS:
            sw = mc.swap_pairs(rng, m, alpha) if m >= 2 else []
            q = sw[0][0] if sw else (rng.choice(alpha),)
            self.q[m] = q
            swaps += [(m, t) for _, t in sw[:6]]
            subs += [(m, mc.embedded(rng, q, alpha, 1, 9)) for _ in range(2)]
        variants = swaps + subs  # 30 + 12: the first member holds one of either kind
        assert len(swaps) == 30 and len(subs) == 12
        self.members, self.planted = [], {m: [] for m in LENGTHS}
        for p in range(16):
            mine = variants[p::16]
            if p % 2 == 0:  # rows of three: the planted word is an alias of a random key
                words = []
                for _, t in mine:
                    words += [rs(rng.randint(5, 20)), t, rs(rng.randint(1, 70))]
                for _ in range(3):
                    words += [rs(rng.randint(5, 20)), rs(rng.randint(1, 70)), None]
                member = Member(words, 3, wide, unique=False)
                for i, (m, t) in enumerate(mine):
                    self.planted[m].append((p, member.kid[tuple(words[3 * i])]))
            else:
                words = [t for _, t in mine] + [rs(rng.randint(1, 70)) for _ in range(4)]
                member = Member(words, 1, wide, unique=True)
                for m, t in mine:
                    self.planted[m].append((p, member.kid[t]))
            self.members.append(member)

    def raw(self, m):
        q = [c + 32 if 65 <= c <= 90 else c for c in self.q[m]]
        return ([32, 9] + q + [32]) if not self.wide else ([32, 0x110000] + q + [9])

    def dispose(self):
        for m in self.members:
            m.ix.dispose()


class View:
    """The first P members as an IndexSet, with the model of its records."""

    def __init__(self, lib, P):
        self.lib, self.members = lib, lib.members[:P]
        self.set = ssl.IndexSet([m.ix for m in self.members])
        self.bases = np.cumsum([0] + [m.nk for m in self.members]).tolist()
        self.total = self.bases[-1]
        assert self.set.num_keys() == self.total

    def gid(self, p, k):
        return self.bases[p] + k

    def rows(self, rng):
        """One row per (query length, count): the planted keys of the members in the set first, then random
        keys with neighbouring records in different members; then the rows of edge ids and special queries."""
        P = len(self.members)
        queries, cn, keys = [], [], []
        for m in LENGTHS:
            mine = [self.gid(p, k) for p, k in self.lib.planted[m] if p < P]
            for c in COUNTS:
                row = list(mine)
                while len(row) < c:
                    p = len(row) % P
                    row.append(self.gid(p, rng.randrange(self.members[p].nk)))
                queries.append(self.lib.raw(m))
                cn.append(c)
                keys.append(row[:c])
        edge = sorted({g for b in self.bases for g in (b - 1, b) if g >= 0} | {self.total - 1, self.total, 0xFFFFFFFF})
        assert len(edge) <= STRIDE
        blank = [32, 9, ord("#"), 32] if not self.lib.wide else [32, 0x110000, 9]
        over = [32] + [self.lib.q[129][i % 129] for i in range(4097)] + [32]
        for q in (self.lib.raw(64), self.lib.raw(129), blank, [], [ord("*")], over):
            queries.append(q)
            cn.append(len(edge))
            keys.append(edge)
        queries.append(self.lib.raw(63))  # a count above the stride reads as the stride
        cn.append(STRIDE + 71)
        keys.append([self.gid(r % P, r % self.members[r % P].nk) for r in range(STRIDE)])
        assert len(sim_ref.normalise(blank, sim_ref.DEFAULT_VALID, self.lib.wide)) == 0
        assert len(sim_ref.normalise(over, sim_ref.DEFAULT_VALID, self.lib.wide)) == 4097
        return queries, cn, keys

    def expect(self, queries, cn, keys, stride, metric, sims_of=metric_ref.record_sims):
        """(sim bits, term ids): every record through the model with its member's keys and term ids."""
        want = np.full((len(queries), stride), FILL, dtype=np.uint32)
        want_t = want.copy()
        per = [([], []) for _ in self.members]
        for i, q in enumerate(queries):
            for r in range(min(cn[i], stride)):
                g = int(keys[i][r])
                if g >= self.total:  # no member: the wildcard's 1.0 or "not computed", no term
                    want[i, r] = bits([1.0 if sim_ref.is_wildcard(q) else -1.0])[0]
                    want_t[i, r] = NO_TERM
                    continue
                p = max(p for p in range(len(self.members)) if self.bases[p] <= g)
                per[p][0].append((tuple(q), self.members[p].key_terms[g - self.bases[p]]))
                per[p][1].append((i, r))
        for member, (pairs, cells) in zip(self.members, per):
            if not pairs:
                continue
            sims, best = sims_of(pairs, metric, member.term_ids, sim_ref.DEFAULT_VALID, self.lib.wide)
            for (i, r), b, t in zip(cells, bits(sims), best):
                want[i, r] = b
                want_t[i, r] = NO_TERM if t is None else member.term_ids[t]
        return want, want_t


@pytest.fixture(scope="module", params=[False, True], ids=["narrow", "wide"])
def planted(request):
    lib = PlantedSet(request.param)
    yield lib
    lib.dispose()


@pytest.mark.parametrize("P", [1, 2, 3, 16])
def test_planted_records_equal_the_per_member_model(planted, P):
    view = View(planted, P)
    try:
        rng = random.Random(0x92 + P)
        queries, cn, keys = view.rows(rng)
        cs = 4 if planted.wide else 1
        if P > 1:  # neighbouring records lie in different members, and a round of 64 meets every member
            row = keys[len(COUNTS) - 1]
            parts = [max(p for p in range(P) if view.bases[p] <= g) for g in row]
            assert sum(a != b for a, b in zip(parts, parts[1:])) >= len(row) // 2 and set(parts) == set(range(P))
        for metric in METRICS:
            want, want_t = view.expect(queries, cn, keys, STRIDE, metric)
            got, got_t = mc.similarity_m(view.set, queries, cn, keys, STRIDE, metric, True, cs)
            mc.check_cells(got, want, f"P={P} metric {metric} sims")
            mc.check_cells(got_t, want_t, f"P={P} metric {metric} terms")
            alone, none = mc.similarity_m(view.set, queries, cn, keys, STRIDE, metric, False, cs)
            assert none is None
            mc.check_cells(alone, want, f"P={P} metric {metric} sims without dTerms")
        # what the rows are meant to hold: the planted pairs tell the metrics apart, ids past the set and
        # the special queries give the fixed values
        lev, _ = view.expect(queries, cn, keys, STRIDE, metric_ref.LEVENSHTEIN)
        osa, _ = view.expect(queries, cn, keys, STRIDE, metric_ref.OSA)
        par, _ = view.expect(queries, cn, keys, STRIDE, metric_ref.PARTIAL)
        assert (lev != osa).any() and (lev != par).any()
        n = len(queries)
        one, zero, none_ = bits([1.0])[0], bits([0.0])[0], bits([-1.0])[0]
        edge = keys[-2]
        past = [r for r, g in enumerate(edge) if g >= view.total]
        assert len(past) == 2 and (lev[n - 7, past] == none_).all() and (lev[n - 7, :past[0]] != none_).all()
        assert (lev[n - 5, :past[0]] == zero).all()                          # m = 0: every term is L insertions
        assert (lev[n - 4, :len(edge)] == one).all() and (lev[n - 3, :len(edge)] == one).all()  # "" and "*"
        assert (lev[n - 2, :len(edge)] == none_).all()                       # 4,097 characters
    finally:
        view.set.dispose()


@pytest.mark.parametrize("p", [0, 1], ids=["several_terms", "one_pair"])
def test_a_member_alone_equals_the_model_on_both_paths(planted, p):
    """ngsSimilarityDeviceM on one member's handle, the body the set runs with the index in registers: keys
    that list their terms (kt_off) and keys with one pair (the key_term map), query lengths at the path
    cut-over (64 | 65) and one past two words, row counts at the round boundary of the short path, and
    ids at and past nKeys, which read nothing."""
    member = planted.members[p]
    cs = 4 if planted.wide else 1
    rng = random.Random(0x94 + p)
    queries, cn, keys = [], [], []
    for m in (1, 64, 65, 129):
        mine = [k for q, k in planted.planted[m] if q == p]
        for c in (1, 64, 65):
            row = mine + [rng.randrange(member.nk) for _ in range(c)]
            queries.append(planted.raw(m))
            cn.append(c)
            keys.append(row[:c])
        queries.append(planted.raw(m))
        edge = [0, member.nk, 0xFFFFFFFF, member.nk - 1]
        cn.append(len(edge))
        keys.append(edge)
    assert any(len(member.key_terms[k]) > 1 for row in keys for k in row if k < member.nk) == (p == 0)
    for metric in METRICS:
        want, want_t = mc.expect_m(queries, cn, keys, 65, member.key_terms, member.term_ids, metric, wide=planted.wide)
        got, got_t = mc.similarity_m(member.ix, queries, cn, keys, 65, metric, True, cs)
        mc.check_cells(got, want, f"member {p} metric {metric} sims")
        mc.check_cells(got_t, want_t, f"member {p} metric {metric} terms")
        alone, none = mc.similarity_m(member.ix, queries, cn, keys, 65, metric, False, cs)
        assert none is None
        mc.check_cells(alone, want, f"member {p} metric {metric} sims without dTerms")
        assert want_t[3][1] == want_t[3][2] == NO_TERM != want_t[3][0]


# ---- NGS_SIM_TOKEN_SORT ---------------------------------------------------------------------------------
def test_token_sort_route_first_flagged_call_included():
    rng = random.Random(0x93)
    rs = lambda n: bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(n))
    names = [b"JOHN SMITH", b"ACME HOLDINGS", b"MARY ANN VON TRAPP", b"GLOBEX   TRADING  CO", b"B  A", b"ZETA"]
    names += [rs(rng.randint(4, 9)) + b" " + rs(rng.randint(3, 8)) for _ in range(10)]
    aliased = []
    for w in names[::2]:
        aliased += [w, b"  ".join(w.split()[::-1]), rs(6) + b" X"]
    lib = type("L", (), {"wide": False})()
    lib.members = [Member([list(w) for w in aliased], 3, False, unique=False),
                   Member([list(w) for w in names[1::2]], 1, False, unique=True)]
    view = View(lib, 2)
    try:
        queries = [list(q) for q in (b"smith, john", b"holdings acme", b"trapp von ann mary", b"co trading globex",
                                     b"a b", b"zeta", b"  SMITH\tJOHN ", b"*", b"", b"   ")]
        row = [view.total + 3]  # an id past the set, then every key, the members in turn
        for k in range(max(m.nk for m in view.members)):
            row += [view.gid(p, k) for p, m in enumerate(view.members) if k < m.nk]
        cn, keys, stride = [len(row)] * len(queries), [row] * len(queries), len(row)
        raw, off = mc.pack(queries, 1)
        s = torch.cuda.Stream()
        mc.ready()
        view.members[0].ix.token_sort_device(raw.data_ptr(), off.data_ptr(), len(queries), raw.data_ptr(), s.cuda_stream)
        s.synchronize()
        for metric in METRICS:  # (the first of these is the members' first flagged call)
            want, want_t = view.expect(queries, cn, keys, stride, metric, token_ref.record_sims)
            plain, _ = view.expect(queries, cn, keys, stride, metric)
            assert (want[:4] != plain[:4]).any(axis=1).all(), "the flag changes nothing in the model"
            got, got_t = mc.similarity_m(view.set, queries, cn, keys, stride, metric | FLAG, True, qbuf=(raw, off))
            mc.check_cells(got, want, f"flagged metric {metric} sims")
            mc.check_cells(got_t, want_t, f"flagged metric {metric} terms")
        # without the flag afterwards: the members' own terms again
        want, want_t = view.expect(queries, cn, keys, stride, metric_ref.OSA)
        got, got_t = mc.similarity_m(view.set, queries, cn, keys, stride, "osa", True)
        mc.check_cells(got, want, "unflagged after flagged sims")
        mc.check_cells(got_t, want_t, "unflagged after flagged terms")
    finally:
        view.set.dispose()
        for m in lib.members:
            m.ix.dispose()


# ---- equality with one index over all rows --------------------------------------------------------------
class Lib:
    """A library as one index and as sets of 2 and 4 parts; in one row range no row has an alias, so the
    member over it has one pair per key."""

    def __init__(self, cls, words, weights, cuts2, cuts4, bare):
        words = list(words)
        for r in range(*bare):
            words[set_corpus.ROW * r + 1] = None
        self.cls, self.words = cls, words
        self.whole = cls(words, set_corpus.ROW, weights, device=0)
        self.sets, self.members = [], []
        for cuts in (cuts2, cuts4):
            ms = [cls(w, set_corpus.ROW, wt, device=0) for w, wt in set_corpus.split(words, weights, cuts)]
            self.members += ms
            self.sets.append(ssl.IndexSet(ms))
            assert sorted(unique_flag(m) for m in ms)[-1] == 1 and unique_flag(ms[0]) == 0
        for ix in self.members + [self.whole]:  # one device copy per distinct term, whatever the number of calls
            ix.term = functools.lru_cache(maxsize=None)(ix.term)
        self.kid = {self.whole.key(k): k for k in range(self.whole.num_keys())}

    def dispose(self):
        for s in self.sets:
            s.dispose()
        for m in self.members + [self.whole]:
            m.dispose()


@pytest.fixture(scope="module")
def narrow_lib():
    words, weights, _ = set_corpus.narrow()
    lib = Lib(ssl.StringIndex, words, weights, (0, 2500, 6000), (0, 2, 2500, 4000, 6000), (2500, 6000))
    yield lib
    lib.dispose()


@pytest.fixture(scope="module")
def wide_lib():
    words, weights, _ = set_corpus.wide()
    lib = Lib(ssl.WideStringIndex, words, weights, (0, 611, 1500), (0, 300, 611, 1000, 1500), (611, 1500))
    yield lib
    lib.dispose()


def fbits(rows, col):
    return [np.array([r[col] for r in row], dtype=np.float32).view(np.uint32).tolist() for row in rows]


def same_records(got, want, where):
    assert [len(r) for r in got] == [len(r) for r in want], f"{where}: counts"
    assert [[r[0] for r in row] for row in got] == [[r[0] for r in row] for row in want], f"{where}: keys"
    assert fbits(got, 1) == fbits(want, 1), f"{where}: score bits"
    assert fbits(got, 2) == fbits(want, 2), f"{where}: sim bits"


def check_terms(rows, queries, metric, flagged, wide, where):
    """Every record's similarity is the model's for the query and the matched term's string."""
    pairs, sims = [], []
    for q, row in zip(queries, rows):
        raw = tuple(sim_ref.units(q, wide))
        for _, _, sim, term in row:
            if term is None:
                assert sim_ref.is_wildcard(raw), f"{where}: a record without a term"
                assert sim == 1.0
                continue
            pairs.append((raw, (tuple(sim_ref.units(term, wide)),)))
            sims.append(sim)
    assert pairs, where
    model = (token_ref if flagged else metric_ref).record_sims(pairs, metric, None, sim_ref.DEFAULT_VALID, wide)[0]
    assert np.array_equal(bits(model), bits(sims)), f"{where}: a matched term does not attain its record's similarity"


def check_score_batch_sim(lib, queries, wide, forms, where):
    for metric in METRICS:
        for flagged in (False, True):
            for limit in (1, 10, 100):
                args = dict(metric=metric, with_terms=True, token_sort=flagged)
                want = lib.whole.score_batch_sim(queries, 0.3, limit, 0.2, **args)
                assert sum(map(len, want)) > len(queries) // 4
                at = f"{where} metric {metric} flag {flagged} limit {limit}"
                check_terms(want, queries, metric, flagged, wide, f"{at} one index")
                for n, form in enumerate(forms):
                    got = form.score_batch_sim(queries, 0.3, limit, 0.2, **args)
                    same_records(got, want, f"{at} set {n}")
                    check_terms(got, queries, metric, flagged, wide, f"{at} set {n}")
                    plain = form.score_batch_sim(queries, 0.3, limit, 0.2, metric=metric, token_sort=flagged)
                    assert plain == [[r[:3] for r in row] for row in got], f"{at} set {n} without terms"


def test_score_batch_set_sim_equals_one_index_narrow(narrow_lib):
    check_score_batch_sim(narrow_lib, set_corpus.narrow_queries(), False, narrow_lib.sets, "narrow")


def test_score_batch_set_sim_equals_one_index_wide_and_utf8(wide_lib):
    qs = set_corpus.wide_queries()
    check_score_batch_sim(wide_lib, qs, True, wide_lib.sets, "wide")
    # the U8 form on the same rows
    words, weights, _ = set_corpus.wide()
    members = [ssl.Utf8StringIndex(w, set_corpus.ROW, wt, device=0)
               for w, wt in set_corpus.split(wide_lib.words, weights, (0, 611, 1500))]
    s = ssl.IndexSet(members)
    try:
        for metric, flagged in ((metric_ref.OSA, False), (metric_ref.PARTIAL, True)):
            want = wide_lib.whole.score_batch_sim(qs, 0.3, 10, 0.2, metric=metric, token_sort=flagged)
            same_records(s.score_batch_sim(qs, 0.3, 10, 0.2, metric=metric, token_sort=flagged), want, f"U8 {metric}")
    finally:
        s.dispose()
        for m in members:
            m.dispose()


def test_effective_limit_above_the_rerank_cap_is_refused(narrow_lib):
    with pytest.raises(ValueError):
        narrow_lib.sets[0].score_batch_sim([b"ABC"], 0.3, 4097)
    assert narrow_lib.sets[0].score_batch_sim([b"ABC"], 0.3, 4096, 0.0) is not None


# ---- the self-join and the clusters ---------------------------------------------------------------------
def test_self_join_set_equals_self_join_across_member_boundaries(narrow_lib):
    lib = narrow_lib
    whole = lib.whole.self_join(0, None, 0.0, 10)  # (threshold 0: full rows, long runs of equal scores)
    for s, ranges in ((lib.sets[0], [(2400, 200)]), (lib.sets[1], [(0, 10), (3990, 20), (5990, 10)])):
        for first, count in ranges:
            got = s.self_join(first, count, 0.0, 10)
            assert len(got) == count and sum(map(len, got)) > count
            for i, row in enumerate(got):
                want = whole[lib.kid[s.key(first + i)]]
                assert [s.key(g) for g, _ in row] == [lib.whole.key(k) for k, _ in want], (first, i)
                assert fbits([row], 1) == fbits([want], 1), (first, i)
                assert first + i not in [g for g, _ in row]
    assert lib.sets[1].self_join(2, 0, 0.3, 10) == []
    with pytest.raises(RuntimeError):
        lib.sets[1].self_join(5999, 2, 0.3, 10)  # past the last key


def by_string(labels, key_of):
    """{key string: the smallest key string of its cluster} and the number of clusters."""
    groups = {}
    for k, lab in enumerate(labels):
        groups.setdefault(lab, []).append(key_of(k))
    out = {}
    for g in groups.values():
        for s in g:
            out[s] = min(g)
    return out, len(groups)


@pytest.mark.parametrize("min_sim,metric", [(None, None), (0.6, "osa")])
def test_dedup_set_equals_dedup_of_one_index(narrow_lib, min_sim, metric):
    lib = narrow_lib
    want, clusters = by_string(lib.whole.dedup(0.3, 10, min_sim, 0, metric), lib.whole.key)
    assert 1 < clusters < lib.whole.num_keys()
    for s in lib.sets:
        for batch in (0, 64):  # one batch, and batches that cross the members' boundaries
            labels = s.dedup(0.3, 10, min_sim, batch, metric)
            got, n = by_string(labels, s.key)
            assert n == clusters and got == want, (batch, n, clusters)
            # the label is the smallest global id of the cluster
            first = {}
            for g, lab in enumerate(labels):
                first.setdefault(lab, g)
            assert all(lab == g for lab, g in first.items())


# ---- device forms against host forms --------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def test_device_forms_equal_host_forms_and_key_queries_span_members(narrow_lib):
    L, s = _native.lib(), narrow_lib.sets[1]
    qs = set_corpus.narrow_queries()[:80]
    nq, limit, stride = len(qs), 10, 10
    metric = metric_ref.OSA
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    counts = np.zeros(nq, dtype=np.uint32)
    keys, terms = np.zeros(nq * stride, dtype=np.uint32), np.zeros(nq * stride, dtype=np.uint32)
    scores, sims = np.zeros(nq * stride, dtype=np.float32), np.zeros(nq * stride, dtype=np.float32)
    L.ngsLastError(1)
    total = L.scoreBatchSetSimM(s.set_id, (C.c_char_p * nq)(*qs), nq, 0.3, limit, metric, 0.3, stride,
                                counts.ctypes.data_as(u32p), keys.ctypes.data_as(u32p), scores.ctypes.data_as(f32p),
                                sims.ctypes.data_as(f32p), terms.ctypes.data_as(u32p))
    assert L.ngsLastError(1) == 0 and total == counts.sum() > 0
    raw, off = mc.pack([list(q) for q in qs], 1)
    d_n, d_k, d_s = dev(np.zeros(nq)), dev(np.zeros(nq * stride)), dev(np.zeros(nq * stride))
    d_v, d_t = mc.filled(nq * stride), mc.filled(nq * stride)
    st = torch.cuda.Stream()
    mc.ready()
    s.search_device(raw.data_ptr(), off.data_ptr(), nq, 0.3, limit, stride, d_n.data_ptr(), d_k.data_ptr(),
                    d_s.data_ptr(), st.cuda_stream)
    s.rerank_device(raw.data_ptr(), off.data_ptr(), nq, stride, d_n.data_ptr(), d_k.data_ptr(), d_s.data_ptr(),
                    d_v.data_ptr(), 0.3, st.cuda_stream, metric=metric, d_terms=d_t.data_ptr())
    st.synchronize()
    assert np.array_equal(host(d_n), counts)
    for i in range(nq):
        c, at = int(counts[i]), i * stride
        for d, h in ((d_k, keys), (d_s, scores.view(np.uint32)), (d_v, sims.view(np.uint32)), (d_t, terms)):
            assert np.array_equal(host(d)[at:at + c], h[at:at + c]), i
    assert (host(d_v)[nq * stride:] == FILL).all() and (host(d_t)[nq * stride:] == FILL).all()

    # ngsSetSelfJoinDevice against selfJoinSet, over a range that spans three members
    first, nk, js = 2495, 1600, 11
    want = s.self_join(first, nk, 0.0, 10)
    assert sum(map(len, want)) > nk
    j_n, j_k, j_s = dev(np.zeros(nk)), dev(np.zeros(nk * js)), dev(np.zeros(nk * js))
    s.self_join_device(first, nk, 0.0, 10, js, j_n.data_ptr(), j_k.data_ptr(), j_s.data_ptr())
    assert L.ngsSetSelfJoinDevice(s.set_id, first, nk, 0.3, 10, js - 1, j_n.data_ptr(), j_k.data_ptr(), j_s.data_ptr(),
                                  None) == -3
    hn, hk, hs = host(j_n), host(j_k), host(j_s)
    for i in range(nk):
        assert hk[i * js:i * js + hn[i]].tolist() == [g for g, _ in want[i]], i
        assert hs[i * js:i * js + hn[i]].tolist() == fbits([want[i]], 1)[0], i

    # the gathered keys are the keys' bytes in order, offsets from 0, at an odd output address
    for first, nk in ((0, 5), (2495, 10), (0, 0), (6000, 0), (3998, 2002)):
        strings = [s.key(first + i) for i in range(nk)]
        nbytes = s.key_query_bytes(first, nk)
        assert nbytes == sum(map(len, strings))
        buf = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        d_off = torch.full((nk + 3,), -1, dtype=torch.int64, device=DEV)
        mc.ready()
        s.key_queries_device(first, nk, buf.data_ptr() + 3, nbytes, d_off.data_ptr())
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert bytes(h[3:3 + nbytes]) == b"".join(strings) and (h[:3] == 0xAB).all() and (h[3 + nbytes:] == 0xAB).all()
        assert d_off.cpu().numpy().tolist() == join_ref.query_offsets([len(x) for x in strings]) + [-1, -1]
    assert L.ngsSetKeyQueriesDevice(s.set_id, 5999, 2, 0x1000, 1 << 20, 0x1000, None) == -3
    assert L.ngsSetKeyQueriesDevice(s.set_id, 0, 5, 0x1000, 3, 0x1000, None) == -3
    assert s.key_query_bytes(5999, 2) == 0


def test_key_queries_of_a_wide_set_are_aligned_characters(wide_lib):
    s = wide_lib.sets[1]
    first, nk = 295, 720  # three boundaries
    strings = [s.key(first + i) for i in range(nk)]
    nbytes = s.key_query_bytes(first, nk)
    assert nbytes == 4 * sum(map(len, strings))
    buf = torch.zeros(nbytes // 4 + 4, dtype=torch.int32, device=DEV)
    d_off = torch.zeros(nk + 1, dtype=torch.int64, device=DEV)
    mc.ready()
    s.key_queries_device(first, nk, buf.data_ptr(), nbytes, d_off.data_ptr())
    torch.cuda.synchronize()
    assert host(buf)[:nbytes // 4].tolist() == [ord(c) for x in strings for c in x]
    assert d_off.cpu().numpy().tolist() == join_ref.query_offsets([len(x) for x in strings], 4)
    assert _native.lib().ngsSetKeyQueriesDevice(s.set_id, first, nk, buf.data_ptr() + 2, nbytes, d_off.data_ptr(),
                                                None) == -3


# ---- a disposed member ------------------------------------------------------------------------------------
def test_a_disposed_member_fails_every_call():
    L = _native.lib()
    words, weights, _ = ssl.synth.gen_corpus(300, seed=17, min_len=5, span=8)
    members = [ssl.StringIndex(words[a:b], 1, weights[a:b], device=0) for a, b in ((0, 100), (100, 200), (200, 300))]
    s = ssl.IndexSet(members)
    try:
        qs = [words[5], words[150]]
        assert [row[0][0] for row in s.score_batch_sim(qs, 0.3, 3)] == qs
        raw, off = mc.pack([list(q) for q in qs], 1)
        d = [dev(np.zeros(40)) for _ in range(5)]
        p = [t.data_ptr() for t in d]
        mc.ready()
        members[1].dispose()
        assert L.ngsSetSimilarityDeviceM(s.set_id, raw.data_ptr(), off.data_ptr(), 2, 3, p[0], p[1], 0, p[2], None, None) == -1
        assert L.ngsSetRerankDeviceM(s.set_id, raw.data_ptr(), off.data_ptr(), 2, 3, p[0], p[1], p[3], p[2], None, 0, 0.0,
                                     None) == -1
        assert L.ngsSetKeyQueriesDevice(s.set_id, 0, 2, p[4], 160, p[3], None) == -1
        assert L.ngsSetSelfJoinDevice(s.set_id, 0, 2, 0.3, 2, 3, p[0], p[1], p[3], None) == -1
        assert L.ngsSetKeyQueryBytes(s.set_id, 0, 2) == 0
        with pytest.raises(RuntimeError):
            s.score_batch_sim(qs, 0.3, 3)
        with pytest.raises(RuntimeError):
            s.self_join(0, 2, 0.3, 3)
        labels = (C.c_uint32 * 300)()
        L.ngsLastError(1)
        assert L.dedupKeysSet(s.set_id, 0.3, 3, 0, -1.0, 0, labels) == 0 and L.ngsLastError(1) != 0
    finally:
        s.dispose()
        for m in members:
            m.dispose()
