"""Every library and query of tests/fast_cases.py is what it claims, proved on the CPU from the rows,
at the skip-table geometry the device build reported (fast_cases.P_GEOM, W_GEOM, D_GEOM; the GPU test
asserts that the index still reports it).
"""
import pytest

import build_ref
import fast_cases as fc
import hash_cases as hc


@pytest.fixture(scope="module")
def P():
    return fc.LibP()


@pytest.fixture(scope="module")
def T():
    return fc.LibT()


@pytest.fixture(scope="module")
def D():
    lib = fc.LibD()
    lib.pairs = fc.d_pairs(lib, build_ref.build([w.encode() for w in lib.words], 3, lib.weights))
    return lib


def test_geometry_is_read_and_a_missing_constant_is_loud():
    assert fc.PART_CAP == 4096 and fc.SLOT_BITS == 13
    with open(fc.COMMON_H) as f:
        text = f.read()
    for name in ("kTableSlots", "kCandCap", "kFastMaxGrams", "kMaxBuckets"):
        with pytest.raises(RuntimeError, match="not found"):
            fc.read_geometry(text.replace(f"{name} =", f"{name}_ ="))


def test_plan_on_a_hand_made_library():
    """plan() on lists small enough to check by hand: 3 buckets of 4 ids at a cap of 4,096."""
    ids = list(range(12))
    lists = {"ABC": ids, "BCD": ids[4:8], "CDE": []}
    p = fc.plan(lists, "ABCDEABC", 4, 3)  # grams ABC BCD CDE DEA EAB ABC
    assert (p.ng, p.p_total, p.btot, p.cls, p.switches) == (2, 16, [3, 5, 5, 3], "one", 0)
    assert p.parts == [(0, 4, False)]
    big = {"ABC": list(range(0, 9000)), "BCD": list(range(3000, 6001))}
    p = fc.plan(big, "ABCD", 4, 3000)
    assert p.btot == [3000, 6000, 3001, 0] and p.cls == "over" and p.switches == 2
    assert p.parts == [(0, 1, False), (1, 2, True), (2, 4, False)]
    p = fc.plan({"ABC": list(range(0, 9000))}, "ABC", 8, 1125)
    assert p.cls == "multi" and p.parts == [(0, 3, False), (3, 6, False), (6, 8, False)]
    assert fc.planner_buckets(1024, 37) == (256, 148) and fc.planner_buckets(64, 625) == (64, 625)


def test_p_rows_and_geometry(P):
    K, span = fc.P_GEOM
    fc.check_geometry(P.n_long, K, span)
    assert P.n_long == len(P.rows) == len(set(P.rows)) == fc.P_ROWS <= 40000
    for i, r in enumerate(P.rows[:fc.P_BASE]):
        if i in P.chain_plan:
            continue
        assert 10 <= len(r) <= 15 and set(r) <= set(fc.NZ if fc.P_BAND[0] <= i < fc.P_BAND[1] else fc.AM), (i, r)
    # the longest list keeps K at 64: more than 16 postings per bucket at K = 32, at most 16 at K = 64
    longest = max(map(len, P.lists.values()))
    assert 16 * 32 + 32 <= longest < 17 * 64


def test_p_hot_strings(P):
    """In its hot bucket every list of a hot string stays under the cap and the ten together are over
    it; in every other bucket all thirty lists together stay well under it."""
    K, span = fc.P_GEOM
    hot_grams = [fc.grams(h) for h in P.hot]
    assert len({g for gs in hot_grams for g in gs}) == 30
    per = {g: [0] * K for gs in hot_grams for g in gs}
    for g, row in per.items():
        for i in P.lists[g]:
            row[i // span] += 1
    for gs, hb in zip(hot_grams, fc.P_HOT_BUCKETS):
        assert hb & 1 and all(per[g][hb] <= fc.PART_CAP for g in gs)
        assert sum(per[g][hb] for g in gs) > fc.PART_CAP
    for b in range(K):
        if b not in fc.P_HOT_BUCKETS:
            assert sum(row[b] for row in per.values()) < fc.PART_CAP // 8, b


def test_p_classes_occur(P):
    for kind, cls, least in (("one", "one", 4), ("band", "one", 3), ("multi", "multi", 4), ("over", "over", 4)):
        got = [P.plans[q].cls for q in P.queries[kind]]
        assert got == [cls] * len(got) and len(got) >= least, (kind, got)
    assert all(len(P.plans[q].parts) >= 3 for q in P.queries["multi"])
    assert max(P.plans[q].switches for q in P.queries["over"]) >= 4
    h0, h1, h2 = P.hot
    assert h0 + h1 + h2 in P.queries["over"] and P.plans[h0 + h1 + h2].switches >= 4
    assert any(len(q) == 140 and any(h in q for h in P.hot) for q in P.queries["over"])
    assert len(P.all_queries()) >= 17
    # the band: its lists are empty over the leading and the trailing buckets, and an A..M query's over
    # the buckets in the middle
    span = fc.P_GEOM[1]
    lo, hi = fc.P_BAND[0] // span, fc.P_BAND[1] // span
    for q in P.queries["band"]:
        bt = P.plans[q].btot
        assert set(q) <= set(fc.NZ) and not any(bt[:lo]) and not any(bt[hi:]) and any(bt[lo:hi])
    for q in P.queries["multi"]:  # (the second chain's planted terms apart)
        assert all(i in P.chain_plan for g in fc.grams(q) for i in P.lists.get(g, ()) if fc.P_BAND[0] <= i < fc.P_BAND[1])


def test_p_long_rows(P):
    r1, r2, r3, v1, v2, v3 = P.long_queries
    assert P.rows[fc.P_BASE:] == P.long_queries and all(len(r) == 257 for r in P.long_queries)
    assert r2 == "A" * 257 and r3 == "AB" * 128 + "A"
    assert P.plans[r1].ng == len(set(fc.grams(r1))) == 255 == fc.MAX_GRAMS
    assert fc.grams(r2).count("AAA") == 255 and sorted(map(fc.grams(r3).count, ("ABA", "BAB"))) == [127, 128]

    def count(q, term):  # searchLong's count of `term` for the query `q`
        return sum(1 for g in fc.grams(q) if g in set(fc.grams(term)))

    for r, v in ((r1, v1), (r2, v2), (r3, v3)):
        assert sum(a != b for a, b in zip(r, v)) == 1
        assert count(r, r) == count(v, v) == 255           # the u8 field at its top value
        assert 252 <= count(v, r) <= 254, count(v, r)      # and a neighbour just below it
    assert [len(q) for q in P.controls] == [258] * 3 and [q[:257] for q in P.controls] == [r1, r2, r3]
    assert len(set(fc.grams(P.controls[0]))) == 256


def test_p_second_chain(P):
    """Planted relative to the second part of a "multi" query: rel = id - lo + 1 homes into the table's
    last four slots, with a base that is not 0."""
    pl = P.plans[P.chain_query]
    assert pl.cls == "multi" and P.chain_query == P.queries["multi"][0]
    b0, b1, over = pl.parts[1]
    lo, hi = b0 * pl.span, min(b1 * pl.span, P.n_long)
    assert lo == P.chain_lo != 0 and not over
    assert len(P.chain_plan) == len(P.chain_rels) >= 6
    assert P.chain_rels == fc.homing(fc.SLOTS - 4, fc.SLOTS - 1, min(hi, fc.P_BASE) - lo)
    own = set(fc.grams(P.chain_query))
    hits = []
    for i, (t, h) in P.chain_plan.items():
        assert P.rows[i] == t and lo <= i < hi and hc.exact_home(i - lo + 1, 13) >= fc.SLOTS - 4
        assert len(set(fc.grams(t)) & own) == h
        hits.append(h)
    assert len(set(hits)) == len(hits) and min(hits) == 3


def test_t_chain(T):
    assert len(T.rows) == fc.T_ROWS == len(set(T.rows))
    assert len(T.tail) == 19 and T.tail[:3] == [986, 2583, 5167]
    assert all(hc.exact_home(i + 1, 13) >= 8188 for i in T.tail)
    assert sorted(T.tail) == [i for i in range(fc.T_ROWS) if hc.exact_home(i + 1, 13) >= 8188]
    assert [hc.exact_home(i + 1, 13) for i in T.displaced] == list(range(11))
    assert [hc.exact_home(i + 1, 13) for i in T.lead] == [8185, 8186, 8187]
    assert len(T.plan) == 19 + 11 + 3 == len(set(T.plan))
    own = fc.grams(T.query)
    assert len(T.query) == 40 and len(set(own)) == 38 and set(T.query) <= set(fc.PLANT)
    hits = sorted(h for _, h in T.plan.values())
    assert hits == list(range(3, 36))  # pairwise different: 3, 4, 5, ... of 38
    for i, (t, h) in T.plan.items():
        assert T.rows[i] == t and set(t) <= set(fc.PLANT) and len(t) >= 6 and len(set(fc.grams(t)) & set(own)) == h
    in_lists = {i for g in own for i in T.lists.get(g, ())}
    assert in_lists == set(T.plan)  # the 33 planted terms and nothing else: no filler shares a gram
    assert all(set(r) <= set(fc.LETTERS) for i, r in enumerate(T.rows) if i not in T.plan)
    pl = fc.plan(T.lists, T.query, 16, 2500)  # one part whatever the geometry: p_total alone decides
    assert pl.cls == "one" and pl.p_total == sum(hits) <= fc.PART_CAP and pl.ng == 38
    # the thresholds cut through the planted counts
    for thr in fc.T_THRESHOLDS[1:]:
        assert 0 < sum(h / 38 >= thr for h in hits) < len(hits)


def test_d_shares(D):
    assert len(D.words) == 3 * fc.D_KEYS == len(set(D.words)) and len(D.queries) >= 17
    _, sp = fc.planner_buckets(*fc.D_GEOM)
    hot = len(D.lists[fc.D_HOT])
    assert hot >= 3 * fc.CAND_CAP and hot > fc.D_KEYS  # in most alias terms
    for q in D.queries:
        assert len(q) == 12 and fc.D_HOT in q
        f = fc.d_facts(D, D.pairs, q, sp)
        assert f["terms"] >= 3 * fc.CAND_CAP
        # a flush frees at least 2,048 - L slots: two flushes or more at every limit, three at 1,024
        assert f["terms"] > 2 * (fc.CAND_CAP - 129) and f["terms"] > 3 * (fc.CAND_CAP - 1024)
        both = f["both"]
        assert both >= 1000, f
        assert 5 * f["larger"] >= both and 5 * f["smaller"] >= both, f
        assert 10 * f["equal"] >= both and 10 * f["negative"] >= both, f
        assert f["split"] >= 10, f


def test_w_classes(P):
    """The wide leg: at gram size 2 the 169 bigrams of each alphabet have lists of thousands of postings,
    K is 256 and a bucket has 156 rows of at most 14 bigrams, 2,184 postings at the very most. So no
    bucket can pass the cap and "over" cannot occur on these rows; "one", "two" and "multi" do."""
    K, span = fc.W_GEOM
    rows = fc.w_rows(P)
    fc.check_geometry(len(rows), K, span)
    assert span * max(len(r) - 1 for r in rows) <= fc.PART_CAP
    lists = fc.lists_of(rows, 2)
    got = {q: fc.plan(lists, q, K, span, 2).cls for q in fc.w_queries(P)}
    assert set(got.values()) == {"one", "two", "multi"}, got
    assert sum(c == "multi" for c in got.values()) >= 4 and len(got) >= 17
