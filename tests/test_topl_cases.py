"""Every library and query of tests/topl_cases.py is what it claims, proved on the CPU from the rows:
the record count of every family, where its targets lie (spread, dense, split), the skip-table geometry
and the flag word the index should report, which branches of wave_select the queried (family, limit)
pairs reach (topl_cases.select_trace), that the oracle (and the compiled reference, where oracle/_ref was
built) agrees with the plain model on every planted query, and that the cases discriminate: a model of
the buffer (refill every 64 records, trim to L, dedup by key keeping the best, prune against tau) gives
the plain answers, and each of its mutants changes the answer of a planted query named here.
"""
import os

import pytest

import topl_cases as tc
from oracle_py import OracleIndex
from tiecheck import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libStringSearchLib.so")
MAKERS = tc.MAKERS
# the flag word (ngsIndexDigest word 16) of every library and twin: 1 keys_unique, 2 tk_identity, 4 tk_monotone, 8 rank lists
FLAGS = {"n1": 7, "n2": 7, "n3": 3, "o1": 3, "o2": 7, "o3": 7, "e1": 7, "e2": 7, "d": 7, "u": 0, "a": 0, "r": 15}
# what a twin's far rows turn off in its base's flag word ("huge" changes w_max alone)
TWIN_OFF = {"alias": 1 | 4, "shared": 1 | 2 | 4, "short": 4, "huge": 0, "weight": 8}


def fam(libs, name):
    """(library name, family, plain model) of the spread or latency family `name`."""
    for lname, (lib, plain) in libs.items():
        if lname != "d":
            for f in lib.families:
                if f.name == name:
                    return lname, f, plain
    raise KeyError(name)


@pytest.fixture(scope="module")
def libs():
    out = {}
    for name, make in MAKERS.items():
        lib = make()
        out[name] = (lib, tc.Plain(lib))
    return out


@pytest.fixture(scope="module")
def R():
    lib = tc.lib_r()
    return lib, tc.Plain(lib)


def records_of(f, lib):
    """The records Q_f has at thresholds 0.3 and 0.2."""
    if f.name == "M":
        return tc.M_KEYS + tc.M_PLAIN     # a key's two M pairs are one record
    if f.name[0] == "A":
        return tc.A_KEYS
    if f.name[0] == "U":
        return f.records
    return f.n + (1 if f.tail != tc.TAIL else 0)


def test_geometry_is_read_and_a_missing_constant_is_loud():
    with open(tc.COMMON_H) as f:
        text = f.read()
    for name in ("kWaveCand", "kWaveMaxLimit", "kDenseBucketLen"):
        with pytest.raises(RuntimeError, match="not found"):
            tc.read_geometry(text.replace(f"{name} =", f"{name}_ ="))
    assert tc.skip_buckets(40000, 1087) == (64, 625) and tc.skip_buckets(36900, 12000)[0] == 1024  # fast_cases' P and D


def test_sizes_and_the_families_named_in_the_issue(libs):
    for name, (lib, _) in libs.items():
        assert lib.n_rows <= 40000
    spread = sorted(f.n for n in ("n1", "n2", "n3") for f in libs[n][0].families if f.name[0] == "N")
    assert spread == list(tc.N_SIZES) == [1, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 320, 600]
    names = {f.name for n in tc.SPREAD for f in libs[n][0].families}
    assert names >= {"Odesc", "Oasc", "Olast", "T2", "Ea", "Eb", "Ec", "Ed", "Ee", "T", "B1", "B2", "B3", "M", "A1", "A2", "P"}
    assert all(len(libs[n][0].families) >= 2 for n in MAKERS)  # every batch mixes families
    assert {1, 2, 63, 64, 65, 127, 128} <= set(tc.E_LIMITS) and tc.A_LIMITS == (1, 2, 64, 128)


def test_hits_and_record_counts(libs):
    """Every target has exactly 3 hits of 10, a filler 1, and nothing else any; so Q_f has its family's
    records at thresholds 0.3 and 0.2 (limit 0), and one per surviving (term, key) pair before the dedup."""
    for name, (lib, plain) in libs.items():
        for f in lib.families:
            assert len(f.query) == 12
            counts = plain.counts(f.query)
            ids = {t: i for i, t in enumerate(plain.terms)}
            targets = {ids[t] for t in f.targets}
            exact = {ids[f.query]} if f.tail != tc.TAIL else set()
            assert {t for t, c in counts.items() if c == 3} == targets, (name, f.name)
            assert {t for t, c in counts.items() if c > 3} == exact and all(counts[t] == 10 for t in exact)
            assert not any(c == 2 for c in counts.values())
            filled = f.n * 3 // 2 if f.name == "A1" else f.n + 10 if f.name == "P" else f.n  # (A1: a set more per key; P: 10 before its own row)
            ones = 3 * tc.FILL * filled if f.fill else 0
            assert sum(c == 1 for c in counts.values()) == ones + (7 * 8 if f.name == "P" else 0), (name, f.name)
            for thr in (0.3, 0.2):
                assert len(plain.answer(f.query, thr, 0)) == records_of(f, lib), (name, f.name, thr)


def test_scores(libs):
    e = {k: fam(libs, k)[1] for k in ("Ea", "Eb", "Ec", "Ed", "Ee", "T")}
    o = {k: fam(libs, k)[1] for k in ("Odesc", "Oasc", "Olast", "T2")}
    for f in [fam(libs, f"N{n}")[1] for n in tc.N_SIZES] + [o[k] for k in ("Odesc", "Oasc", "Olast")]:
        assert len(set(f.scores())) == f.n                       # distinct scores
    assert o["Odesc"].scores() == sorted(o["Odesc"].scores(), reverse=True)
    assert o["Oasc"].scores() == sorted(o["Oasc"].scores())
    assert min(o["Olast"].scores()[300:]) > max(o["Olast"].scores()[:300])  # the best 300 arrive last
    for k in ("Ea", "Eb", "T"):
        assert len(set(e[k].scores())) == 1
    assert e["Ea"].weights[0] == tc.W_MAX == tc.w_max(libs["e1"][1].m) == tc.w_max(libs["u"][1].m)
    assert e["T"].weights[0] == tc.W_MAX == tc.w_max(libs["e2"][1].m)
    assert o["T2"].weights[0] == tc.O_WMAX == tc.w_max(libs["o1"][1].m)  # bound fl(w_max * s) == the records' score
    runs = sorted(set(e["Ec"].scores()), reverse=True)
    assert [e["Ec"].scores().count(s) for s in runs] == [100, 50, 50, 400]
    ed = sorted(e["Ed"].scores())
    assert [b - a for a, b in zip(ed, ed[1:])] == [1] * 149      # one ulp apart
    ee = e["Ee"].scores()
    assert ee.count(0) == 20 and len({s >> 23 for s in ee if s}) == 80  # +0 and 80 exponents
    # P: six keys each at 7 scores around 100, some below, some at, some above it; the query is a key
    p = fam(libs, "P")[1].scores()
    h = tc.bits(100.0)
    assert sum(s == h for s in p) == 6 and sum(h - 8 <= s < h for s in p) >= 12 and sum(h < s <= h + 8 for s in p) >= 12
    assert fam(libs, "P")[1].query.encode() in libs["n3"][1].keys


def test_spread_dense_and_split(libs):
    for name, (lib, plain) in libs.items():
        m = plain.m
        K, span = tc.skip_buckets(m.n_long, max(map(len, m.lists)))
        ids = {t: i for i, t in enumerate(plain.terms)}
        first = {f.name: [ids[t] for t in f.targets] for f in lib.families}
        for f in lib.families:
            t_ids = sorted(first[f.name])
            tset = set(t_ids)
            if lib.dense:
                if f.n >= 192:  # runs of 192 consecutive ids or more: a part of whole 80-id buckets has 80 of them or more
                    for run in ((t_ids[:f.n // 2], t_ids[f.n // 2:]) if f.split else (t_ids,)):
                        assert run == list(range(run[0], run[0] + len(run))) and len(run) >= 192 and span <= 96, (name, f.name)
                continue
            if name == "u" or not f.fill:
                assert name == "u" or f.n <= tc.PART_TARGETS or f.name == "M"
                continue  # the latency path alone, or 21 targets at most (M: 62 survivors, see lib_m)
            for g in tc.grams(f.prefix):  # no part's worth of one list has more than 21 targets (3 entries each)
                lst = plain.lists[g]
                hit = [i in tset for i in lst]
                run = sum(hit[:tc.PART_POSTINGS])
                worst = run
                for j in range(tc.PART_POSTINGS, len(hit)):
                    run += hit[j] - hit[j - tc.PART_POSTINGS]
                    worst = max(worst, run)
                assert worst <= tc.PART_TARGETS and 3 * worst <= 64, (name, f.name, worst)
            assert tc.part_entries(plain, f.query, 3) <= 64 and tc.part_entries(plain, f.query, 2) <= 64, (name, f.name)
            per_bucket = {}
            for i in t_ids:
                per_bucket[i // span] = per_bucket.get(i // span, 0) + 1
            assert max(per_bucket.values()) <= 64, (name, f.name)
            if f.split:  # every other family lies between the halves
                others = [i for g in lib.families if not g.split for i in first[g.name]]
                half = f.n // 2 if name != "a" else tc.A_KEYS
                a, b = [ids[t] for t in f.targets[:half]], [ids[t] for t in f.targets[half:]]
                assert not others or max(a) < min(others) and max(others) < min(b), (name, f.name)
                assert min(a) // span == 0 and max(b) // span >= (m.n_long - 1) // span - 1 and min(b) // span - max(a) // span >= K // 4
    # the latency path's tier 1b stays one wave per query on library u alone (n_buckets / 8 <= 1)
    geo = {name: tc.skip_buckets(p.m.n_long, max(map(len, p.m.lists))) for name, (_, p) in libs.items()}
    assert geo["u"][0] == 8 and all(g[0] >= 16 for k, g in geo.items() if k != "u"), geo


def test_key_ranks(libs):
    lib, plain = libs["e1"]
    rank = {bytes(k).decode(): r for r, k in enumerate(plain.m.keys)}
    ea = [rank[t] for t in lib.families[0].targets]
    assert len({r >> 7 for r in ea}) == 1                     # one aligned block of 128
    eb = [rank[t] for t in lib.families[1].targets]
    assert max(eb) >> 15 == 1 and min(eb) >> 15 == 0          # differing bits up to bit 15
    assert plain.m.keys == [k for k in plain.m.keys if len(k) == 9]
    lib, plain = libs["o1"]
    t2 = lib.families[-1]
    assert plain.keys[0] == t2.targets[-1].encode() and plain.terms.index(t2.targets[-1]) > plain.terms.index(t2.targets[-2])


def test_flag_words(libs, R):
    for name, (lib, plain) in list(libs.items()) + [("r", R)]:
        assert tc.flag_word(plain.m) == FLAGS[name], name
    for base, kind in tc.TWIN_CASES:
        t = tc.twin(libs[base][0], kind)
        off = TWIN_OFF[kind]
        assert tc.flag_word(t.model()) == FLAGS[base] & ~off, t.name
        assert kind == "huge" or FLAGS[base] & off, t.name          # a twin that flips nothing proves nothing
        assert (tc.w_max(t.model()) > 1e29) == (kind == "huge")
    for base in ("e1", "e2"):
        neg = tc.negative(libs[base][0])
        assert tc.flag_word(neg.model()) == FLAGS[base] and tc.w_max(neg.model()) == 0.0
    assert tc.flag_word(tc.twin(R[0], "weight").model()) == FLAGS["r"] & ~TWIN_OFF["weight"]
    assert tc.flag_word(tc.lib_r(-2.0).model()) == 15
    # the twins meet refills: their bases hold families of more than 256 records
    assert all(max(f.n for f in libs[b][0].families) > tc.CAND for b in ("e2", "o1", "n1", "a"))


def test_select_branches(libs):
    """wave_select on the whole record set of a family of at most 256 records (unique keys, a RADIX route:
    the final wave_flush runs exactly one wave_select(n_f, L)), at the limits library e is queried at."""
    seen = {"first": set(), "last": set(), "lane": set(), "j": set(), "passes": set(), "sh0": set()}
    for lib, plain, f in [(libs[n][0], libs[n][1], f) for n in ("e1", "o2", "o3") for f in libs[n][0].families]:
        if f.n > tc.CAND:
            continue
        recs = [tc.record(sb, r) for sb, r in plain.best(f.query, 0.2)]
        assert len(recs) == f.n
        for L in tc.E_LIMITS:
            if L >= f.n:
                continue
            passes, kth = tc.select_trace(recs, L)
            assert kth == sorted(recs)[L - 1]
            seen["passes"].add((min(len(passes), 4), f.name))
            for p in passes:
                for k in ("first", "last"):
                    if p[k] and p["in_bin"] > 1:
                        seen[k].add(f.name)
                seen["lane"].add(p["lane"])
                if p["lane"] == 0:
                    seen["j"].add(p["j"])
                if p["top"] < 7:
                    seen["sh0"].add(f.name)
    assert seen["first"] and seen["last"], seen          # k == excl + 1 and k == incl in a bin of several records
    assert {0, 63} <= seen["lane"] and seen["j"] == {0, 1, 2, 3}, seen
    assert {n for n, _ in seen["passes"]} >= {1, 2, 4}, seen["passes"]
    assert (1, "B1") in seen["passes"] and (4, "B3") in seen["passes"]
    assert "Ea" in seen["sh0"]                            # the tied records differ only below bit 7: sh = 0


def _keys(plain, recs):
    return [(plain.keys[r], sb) for sb, r in recs]


def test_buffer_model_gives_the_plain_answers(libs):
    refills = {}
    for name, (lib, plain) in libs.items():
        for f in lib.families:
            for thr in (0.3, 0.2):
                terms = tc.arrival(plain, f.query, thr)
                for L in tc.limits_of(name):
                    got, nref = tc.buffer_model(terms, L)
                    assert _keys(plain, got) == plain.answer(f.query, thr, L), (name, f.name, thr, L)
                    refills[f.name] = nref
    # 257 records and more refill the buffer at least once; up to 256 never do
    for n in tc.N_SIZES:
        assert (refills[f"N{n}"] >= 1) == (n >= 257), n
    assert refills["M"] >= 1 and refills["A1"] >= 2 and refills["A2"] >= 2 and refills["Uo"] >= 1 and refills["Ut"] >= 1


# mutation -> (library, family, threshold, limit) whose answer it changes
CAUGHT_BY = {"lt_kth": ("n1", "N600", 0.3, 64), "tie_out": ("o1", "T2", 0.3, 64), "prune_le": ("o1", "T2", 0.3, 64),
             "dedup_first": ("a", "A1", 0.3, 128)}
# ... and the unsliced route's own families are caught the same way
CAUGHT_UNSLICED = {"lt_kth": "Uo", "tie_out": "Ut", "prune_le": "Ut"}


@pytest.mark.parametrize("mutation", sorted(CAUGHT_BY))
def test_each_mutant_is_caught(libs, mutation):
    name, fam, thr, L = CAUGHT_BY[mutation]
    lib, plain = libs[name]
    f = next(f for f in lib.families if f.name == fam)
    terms = tc.arrival(plain, f.query, thr)
    good, _ = tc.buffer_model(terms, L)
    bad, _ = tc.buffer_model(terms, L, mutation=mutation)
    assert _keys(plain, good) == plain.answer(f.query, thr, L) and bad != good, (mutation, fam)
    if mutation in CAUGHT_UNSLICED:
        lib, plain = libs["u"]
        f = next(f for f in lib.families if f.name == CAUGHT_UNSLICED[mutation])
        terms = tc.arrival(plain, f.query, thr)
        assert tc.buffer_model(terms, L, mutation=mutation)[0] != tc.buffer_model(terms, L)[0], (mutation, f.name)


def test_rank_lists_and_the_kset_mutant(R):
    lib, plain = R
    for kind, q in lib.queries.items():
        g = tc.grams(q)
        multi = [t for t, c in plain.counts(q).items() if c >= 2]
        ones = [t for t, c in plain.counts(q).items() if c == 1]
        assert len(multi) == tc.R_MULTI[kind] and len(ones) == sum(tc.r_lengths(kind))
        assert [len(plain.lists[x]) for x in g] == [n + (len(multi) if j < 3 else 0) for j, n in enumerate(tc.r_lengths(kind))]
        # tier 1a counts the query at cmin 2 without handing it over: every part fits the first list's cap
        assert tc.part_entries(plain, q, 2, tc.R_PART, g[:1]) <= 64
        first = sorted(plain.m.tk[t][0][0] for t in plain.lists[g[0]])[:128]
        assert sum(plain.m.tk[t][0][0] in first for t in multi) >= min(len(multi), 8)  # stand-ins inside the prefix
    assert len(tc.R_LENGTHS) == 10 > 8  # more lists than kRankLoads
    assert min(tc.R_LENGTHS) < 63 and {63, 64, 65, 127, 128, 129} <= set(tc.R_LENGTHS)
    for kind, q in lib.queries.items():
        for L in tc.LIMITS:
            assert tc.rank_prefix_model(plain, q, L) == plain.answer(q, 0.0, L), (kind, L)
    assert tc.R_MULTI["full"] > tc.MAX_LIMIT  # cand_n > L on entry at every limit
    q = lib.queries["some"]  # named: the query whose answer the kset mutant changes
    assert tc.rank_prefix_model(plain, q, 64, skip_kset=True) != plain.answer(q, 0.0, 64)


def _oracle(lib):
    return OracleIndex(lib.encoded(), lib.row_size, lib.weights)


def test_oracle_agrees_with_the_plain_model(libs, R):
    for name, (lib, plain) in libs.items():
        oi = _oracle(lib)
        for f in lib.families:
            for thr in (0.3, 0.2):
                for L in tc.limits_of(name) + (0,):
                    got, amb = oi.score_amb(f.query.encode(), thr, L)
                    assert not amb, (name, f.name)
                    assert [(k, tc.bits(s)) for k, s in got] == plain.answer(f.query, thr, L), (name, f.name, thr, L)
        oi.close()
    for weight in (None, -2.0):
        lib = tc.lib_r(weight)
        plain, oi = tc.Plain(lib), _oracle(lib)
        for q in lib.queries.values():
            for L in tc.LIMITS:
                got, amb = oi.score_amb(q.encode(), 0.0, L)
                assert not amb and [(k, tc.bits(s)) for k, s in got] == plain.answer(q, 0.0, L), (weight, q, L)
        oi.close()


def test_twins_answer_like_their_base_in_the_oracle(libs):
    bases = {}
    for name, kind in tc.TWIN_CASES:
        lib = libs[name][0]
        if name not in bases:
            bases[name] = _oracle(lib)
        oi = _oracle(tc.twin(lib, kind))
        for f in lib.families:
            for L in (1, 64, 128):
                q = f.query.encode()
                assert oi.score(q, 0.3, L) == bases[name].score(q, 0.3, L), (name, kind, f.name, L)
        oi.close()
    for oi in bases.values():
        oi.close()


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built")
def test_compiled_reference_agrees(libs, R):
    """The compiled reference on every planted query (thresholds 0.3 and 0.2; family R at 0), tie-aware, with
    no query skipped as order-dependent."""
    from test_ref_fuzz import LiveReference
    cases = [(name, lib, plain, [f.query for f in lib.families], (0.3, 0.2), tc.limits_of(name))
             for name, (lib, plain) in libs.items()]
    cases.append(("r", R[0], R[1], list(R[0].queries.values()), (0.0,), tc.LIMITS))
    skipped = checked = 0
    for name, lib, plain, queries, thresholds, limits in cases:
        ref = LiveReference()
        ref.open(lib.encoded(), lib.row_size, lib.weights if lib.weights is not None else [1.0] * len(lib.words))
        oi = _oracle(lib)
        for query in queries:
            q = query.encode()
            for thr in thresholds:
                _, amb = oi.score_amb(q, thr, 0)
                skipped += amb
                full = ref.full(q, thr, ())
                for L in limits:
                    check(plain.answer(query, thr, L), ref.count(q, thr, L), [k for k, _ in full],
                          [tc.bits(s) for _, s in full], f"{name} {query} thr {thr} limit {L}")
                    checked += 1
        ref.close()
        oi.close()
    assert skipped == 0 and checked == sum(len(c[3]) * len(c[4]) * len(c[5]) for c in cases)
