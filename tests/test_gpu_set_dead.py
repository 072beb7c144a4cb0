"""Dead keys in index sets on the GPU: ngsDropDeadDevice over planted blocks against the
model of tests/dead_ref.py, and sets of real indexes after the removal plans of tests/dead_corpus.py
against the oracle over the live rows and against a fresh index over the live rows. Every comparison is
exact: key strings or ids, order, fp32 bits."""
import ctypes as C

import numpy as np
import pytest

import dead_cases
import dead_corpus
import dead_ref
import set_corpus
from oracle_py import OracleIndex, OracleIndexG

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64
CANARY = 0x5A5AA5A5
CASES = dead_cases.cases()
GRID = [(t, l) for t in set_corpus.THRESHOLDS for l in set_corpus.LIMITS]
ROW = set_corpus.ROW


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def padded(a):
    """`a` between two runs of canaries: (the whole tensor, the address of a[0])."""
    whole = np.full(len(a) + 2 * PAD, CANARY, dtype=np.uint32)
    whole[PAD:PAD + len(a)] = a
    t = dev(whole)
    return t, t.data_ptr() + 4 * PAD


def inner(t, what):
    h = host(t)
    assert (h[:PAD] == CANARY).all() and (h[len(h) - PAD:] == CANARY).all(), f"a write outside {what}"
    return h[PAD:len(h) - PAD]


# ---- 1. planted blocks, no handle -----------------------------------------------------------------------
def run_drop(block, limit, with_short=True, n=None):
    """ngsDropDeadDevice on padded copies of the block -> (counts, rows, short rows), after the checks
    that nothing outside the block, nothing past a row's new count and nothing of the mask changed."""
    n = block["n"] if n is None else n
    stride = block["stride"]
    c, k, s = padded(block["counts"]), padded(block["keys"]), padded(block["scores"])
    m = padded(block["dead"]) if block["dead"] is not None else (None, 0)
    sh = padded(np.array([5], dtype=np.uint32)) if with_short else (None, 0)
    ssl.drop_dead_device(c[1], k[1], s[1], n, stride, m[1], block["n_keys"], limit, sh[1])
    torch.cuda.synchronize()
    counts, keys, scores = inner(c[0], "the counts"), inner(k[0], "the keys"), inner(s[0], "the scores")
    if m[0] is not None:
        assert np.array_equal(inner(m[0], "the mask"), block["dead"]), "the mask changed"
    short = int(inner(sh[0], "the short counter")[0]) - 5 if with_short else None
    assert np.array_equal(counts[n:], block["counts"][n:])
    rows = []
    for i in range(block["n"]):
        at = i * stride
        new = int(counts[i]) if i < n else 0
        assert new <= min(int(block["counts"][i]), stride)
        # the cells past the new count are the input's: no write there (rows past n are untouched)
        assert np.array_equal(keys[at + new:at + stride], block["keys"][at + new:at + stride]), f"row {i}: keys past its count"
        assert np.array_equal(scores[at + new:at + stride], block["scores"][at + new:at + stride]), f"row {i}"
        rows.append(list(zip(keys[at:at + new].tolist(), scores[at:at + new].tolist())))
    return counts[:n].tolist(), rows[:n], short


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_drop_of_planted_blocks_equals_the_model(case):
    name, block, limits = case
    assert block["n"] <= 10
    for limit in limits:
        want_c, want, want_short = dead_ref.drop(block, limit)
        got_c, got, short = run_drop(block, limit)
        assert got_c == want_c.tolist(), (name, limit, got_c, want_c.tolist())
        for i in range(block["n"]):
            assert got[i] == want[i], (name, limit, i, got[i][:4], want[i][:4])
        assert short == want_short, (name, limit)


def test_drop_without_a_short_counter_without_rows_and_a_repeat():
    by = {c[0]: c[1] for c in CASES}
    for name, limit in (("wave-random", 100), ("group-random", 164)):  # one wave, a workgroup
        block = by[name]
        want_c, want, _ = dead_ref.drop(block, limit)
        runs = [run_drop(block, limit, with_short=False) for _ in range(2)]  # dShort NULL; reproducible bit for bit
        assert runs[0] == runs[1] and runs[0][0] == want_c.tolist() and runs[0][1] == want
    got_c, got, short = run_drop(by["group-random"], 10, n=0)  # n = 0: nothing is written or counted
    assert got_c == [] and short == 0
    got_c, got, short = run_drop(by["group-alternate"], 10, n=3)  # the rows past n stay as they were
    assert got_c == dead_ref.drop(by["group-alternate"], 10)[0].tolist()[:3]


# ---- sets of real indexes -----------------------------------------------------------------------------
class Lib:
    """The narrow library in an IndexSet of 3 members; per plan, a fresh index and the oracle over the
    live rows. names[g] is the key string of global id g before anything was removed."""

    def __init__(self):
        self.words, self.weights, self.cuts = set_corpus.narrow()
        self.members = [ssl.StringIndex(w, ROW, wt, device=0)
                        for w, wt in set_corpus.split(self.words, self.weights, self.cuts)]
        self.set = ssl.IndexSet(self.members)
        self.names = [self.set.key(g) for g in range(self.set.num_keys())]
        self.ids = {k: g for g, k in enumerate(self.names)}
        assert len(self.ids) == len(self.names) == 6000
        self.plan, self.live, self._want = None, {}, {}

    def use(self, plan):
        """The set with exactly `plan`'s keys dead (None: none) -> the dead global ids."""
        if plan != self.plan:
            self.set.restore(self.set.dead_keys())
            if plan is not None:
                removed = dead_corpus.plan(plan)
                assert self.set.remove([self.ids[k] for k in removed]) == len(removed)
            self.plan = plan
        dead = self.set.dead_keys()
        assert self.set.live_keys() == 6000 - len(dead)
        return dead

    def fresh(self, plan):
        """(a fresh index, the oracle) over the rows `plan` leaves."""
        if plan not in self.live:
            w, wt = dead_corpus.live_rows(self.words, self.weights, dead_corpus.plan(plan) if plan else ())
            self.live[plan] = (ssl.StringIndex(w, ROW, wt, device=0), OracleIndex(w, ROW, wt))
        return self.live[plan]

    def want(self, plan, thr, limit):
        if (plan, thr, limit) not in self._want:
            oracle = self.fresh(plan)[1]
            self._want[plan, thr, limit] = [oracle.score(q, thr, limit) for q in set_corpus.narrow_queries()]
        return self._want[plan, thr, limit]

    def dispose(self):
        self.set.dispose()
        for m in self.members + [ix for ix, _ in self.live.values()]:
            m.dispose()
        for _, o in self.live.values():
            o.close()


@pytest.fixture(scope="module")
def lib():
    out = Lib()
    yield out
    out.dispose()


def batch_ids(s, queries, thr, limit):
    """scoreBatchSet through ctypes -> per query [(global id, score)]."""
    L, nq = _native.lib(), len(queries)
    stride = max(1, min(limit or dead_ref.LIMIT_ALL, s.num_keys()))
    counts = (C.c_uint32 * nq)()
    keys = (C.c_uint32 * (nq * stride))()
    scores = (C.c_float * (nq * stride))()
    L.ngsLastError(1)
    total = L.scoreBatchSet(s.set_id, (C.c_char_p * nq)(*queries), nq, thr, limit, stride, counts, keys, scores)
    assert L.ngsLastError(1) == 0 and total == sum(counts)
    return [[(keys[i * stride + j], scores[i * stride + j]) for j in range(counts[i])] for i in range(nq)]


def same(got, want, where):
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        gk, wk = [r[0] for r in g], [r[0] for r in w]
        assert gk == wk, f"{where}: query {i}: keys {gk[:4]} vs {wk[:4]} ({len(gk)} vs {len(wk)})"
        for col in range(1, len(g[0]) if g else 1):
            gs = np.array([r[col] for r in g], dtype=np.float32).view(np.uint32)
            ws = np.array([r[col] for r in w], dtype=np.float32).view(np.uint32)
            assert np.array_equal(gs, ws), f"{where}: query {i}: bits of column {col} differ"


# ---- 2. end to end, narrow ------------------------------------------------------------------------------
@pytest.mark.parametrize("thr,limit", GRID)
@pytest.mark.parametrize("plan", dead_corpus.PLANS)
def test_narrow_set_with_dead_keys_equals_the_oracle_and_a_fresh_index(lib, plan, thr, limit):
    qs = set_corpus.narrow_queries()
    dead = set(lib.use(plan))
    assert len(dead) == len(dead_corpus.plan(plan))
    raw = batch_ids(lib.set, qs, thr, limit)
    # every returned id is live and is the old global id of its string
    assert not any(g in dead for row in raw for g, _ in row)
    got = [[(lib.names[g], s) for g, s in row] for row in raw]
    same(got, lib.want(plan, thr, limit), f"plan {plan}: set vs oracle at ({thr}, {limit})")
    same(got, lib.fresh(plan)[0].score_batch(qs, thr, limit), f"plan {plan}: set vs fresh index at ({thr}, {limit})")
    same(lib.set.score_batch(qs, thr, limit), got, f"plan {plan}: score_batch vs scoreBatchSet")


def test_the_plans_cut_what_they_are_meant_to(lib):
    qs = set_corpus.narrow_queries()
    fam = dead_corpus.family()
    # (b): the limit cuts the tie class at another place: the first 10 live members are the odd ones
    lib.use("b")
    assert [k for k, _ in lib.set.score_batch([set_corpus.TIE_QUERY], 0.0, 10)[0]] == fam[1:20:2]
    # (c): a query whose exact match is dead is promoted no longer
    lib.use("c")
    promoted = [q for q in qs if q in set(dead_corpus.plan("c"))]
    for q, row in zip(promoted, lib.set.score_batch(promoted, 0.3, 1)):
        assert not row or row[0][0] != q, q
    # (d): the first member is wholly dead and the set answers from the others
    dead = lib.use("d")
    assert dead == [0, 1] and lib.members[0].num_keys() == 2
    assert not lib.set.is_live(0) and not lib.set.is_live(1) and lib.set.is_live(2)
    # a wholly dead member can give no record: it is not searched, and with no other dead key nothing is dropped
    before = lib.set.dead_stats()
    got = lib.set.score_batch(qs, 0.3, 10)
    assert lib.set.dead_stats() == before
    same(got, lib.want("d", 0.3, 10), "plan d without a drop launch")


def test_over_fetch_grows_in_plan_e_and_not_in_plan_a(lib):
    """TIE_QUERY at limit 10 meets more dead records in the second member than the first over-fetch
    holds: that member is searched again. A tenth dead at random never fills an over-fetch."""
    qs = set_corpus.narrow_queries()
    lib.use("a")
    before = lib.set.dead_stats()
    for thr, limit in GRID:
        lib.set.score_batch(qs, thr, limit)
    after = lib.set.dead_stats()
    assert after["re_searches"] == before["re_searches"]
    assert after["drop_launches"] == before["drop_launches"] + len(GRID)  # one launch a search
    assert lib.set.dead_stats()["max_over_fetch"] >= dead_ref.first_fetch(500, 100)
    # (e) on a set of its own over the same members: another mask, and counters that start at zero
    s = ssl.IndexSet(lib.members)
    try:
        removed = [lib.ids[k] for k in dead_corpus.plan("e")]
        assert s.remove(removed) == 150 and lib.set.dead_keys() != s.dead_keys()
        assert s.dead_stats() == {"drop_launches": 0, "re_searches": 0, "max_over_fetch": 0}
        got = s.score_batch([set_corpus.TIE_QUERY], 0.0, 10)
        assert [k for k, _ in got[0]] == dead_corpus.family()[150:160]
        d2 = sum(1 for g in removed if 2 <= g < 2500)  # the second member's dead keys: all its family
        e0 = dead_ref.first_fetch(d2, 10)
        assert d2 > e0 > 150 - d2
        # the second member's first block of 10 + E0 records was all dead: searched again once, at
        # E = min(d2, 4 x E0); the third member's block held live family keys
        assert s.dead_stats() == {"drop_launches": 2, "re_searches": 1, "max_over_fetch": min(d2, dead_ref.GROWTH * e0)}
    finally:
        s.dispose()


def test_restore_gives_back_the_parents_answers_and_launches_no_drop(lib):
    qs = set_corpus.narrow_queries()
    lib.use("a")
    n = len(lib.set.dead_keys())
    assert lib.set.restore(lib.set.dead_keys()) == n and lib.set.dead_keys() == [] and lib.set.live_keys() == 6000
    lib.plan = None
    before = lib.set.dead_stats()
    for thr, limit in ((0.0, 10), (0.3, 100), (0.3, 0)):
        got = lib.set.score_batch(qs, thr, limit)
        same(got, lib.want(None, thr, limit), f"restored vs oracle at ({thr}, {limit})")
        same(got, lib.fresh(None)[0].score_batch(qs, thr, limit), f"restored vs one index at ({thr}, {limit})")
    lib.set.self_join(0, 50, 0.3, 10)
    assert lib.set.dead_stats() == before  # no drop kernel, no re-search: what a set without dead keys launches


# ---- 3. arguments ---------------------------------------------------------------------------------------
def test_remove_arguments_append_and_two_sets():
    L = _native.lib()
    words, weights, _ = ssl.synth.gen_corpus(400, seed=23, min_len=5, span=8)
    a = ssl.StringIndex(words[:200], 1, weights[:200], device=0)
    b = ssl.StringIndex(words[200:300], 1, weights[200:300], device=0)
    s, t = ssl.IndexSet([a, b]), ssl.IndexSet([a])
    c = None
    try:
        n = s.num_keys()
        assert s.remove([3, 7, 3, 3, 7]) == 2 and s.dead_keys() == [3, 7]      # duplicates count once
        assert s.remove([7]) == 0 and s.restore([5]) == 0                      # already dead, already live
        before = s.dead_keys()
        with pytest.raises(IndexError):
            s.remove([1, n])                                                   # an id past the set: nothing changed
        assert s.dead_keys() == before and s.is_live(1)
        with pytest.raises(IndexError):
            s.restore([3, 0xFFFFFFFF])
        assert s.dead_keys() == before
        assert L.ngsSetRemove(s.set_id, None, 1) == -3 and L.ngsSetRemove(s.set_id, None, 0) == 0
        with pytest.raises(IndexError):
            s.is_live(n)
        out = (C.c_uint32 * 1)()
        assert L.ngsSetDeadKeys(s.set_id, out, 1) == 2 and out[0] == 3         # the first `cap` of them
        # the member searched directly still returns the removed key, and so does the other set
        k3 = s.key(3)
        assert not s.is_live(3) and s.num_keys() == n and s.live_keys() == n - 2
        assert a.score_batch([k3], 0.3, 1) == [[(k3, 100.0)]] and t.score_batch([k3], 0.3, 1) == [[(k3, 100.0)]]
        assert k3 not in [k for k, _ in s.score_batch([k3], 0.0, 0)[0]]
        assert t.dead_keys() == [] and t.remove([5]) == 1 and s.is_live(5) and not t.is_live(5)
        k5 = t.key(5)
        assert s.score_batch([k5], 0.3, 1) == [[(k5, 100.0)]] and t.score_batch([k5], 0.3, 1)[0][:1] != [(k5, 100.0)]
        # remove after add: ids stay, the new member's keys can die, an update is remove + append
        c = s.append(words[300:], 1, weights[300:])
        assert s.dead_keys() == [3, 7] and s.num_keys() == n + c.num_keys()
        g = n + 4
        kg = s.key(g)
        assert s.score_batch([kg], 0.3, 1) == [[(kg, 100.0)]]
        assert s.remove([g, 3]) == 1 and s.dead_keys() == [3, 7, g]
        assert kg not in [k for k, _ in s.score_batch([kg], 0.0, 0)[0]]
        gone = (k3, s.key(7), kg)
        whole = ssl.StringIndex([w for w in words if w not in gone], 1,
                                [x for w, x in zip(words, weights) if w not in gone], device=0)
        try:
            qs = words[::7] + [k3, kg, b"", b"*", b"AB"]
            for thr, limit in ((0.0, 10), (0.3, 0)):
                same(s.score_batch(qs, thr, limit), whole.score_batch(qs, thr, limit), f"after add at ({thr}, {limit})")
        finally:
            whole.dispose()
    finally:
        s.dispose()
        t.dispose()
        for ix in (a, b, c):
            if ix is not None:
                ix.dispose()


# ---- 4. wide / UTF-8 ------------------------------------------------------------------------------------
def test_utf8_set_with_dead_keys_equals_the_oracle_and_a_fresh_index():
    words, weights, cuts = set_corpus.wide()
    members = [ssl.Utf8StringIndex(w, ROW, wt, device=0) for w, wt in set_corpus.split(words, weights, cuts)]
    s = ssl.IndexSet(members)
    w, wt = dead_corpus.live_rows(words, weights, dead_corpus.wide_plan())
    fresh, oracle = ssl.Utf8StringIndex(w, ROW, wt, device=0), OracleIndexG(w, ROW, wt, g=2, wide=True)
    try:
        ids = {s.key(g): g for g in range(s.num_keys())}
        removed = dead_corpus.wide_plan()
        assert s.remove([ids[k] for k in removed]) == len(removed) == s.num_keys() - fresh.num_keys()
        qs = set_corpus.wide_queries()
        for thr, limit in GRID:
            got = s.score_batch(qs, thr, limit)  # scoreBatchSetU8
            same(got, [oracle.score(q, thr, limit) for q in qs], f"U8 set vs oracle at ({thr}, {limit})")
            same(got, fresh.score_batch(qs, thr, limit), f"U8 set vs fresh index at ({thr}, {limit})")
        # the wide tie family: every second member is dead, the limit cuts inside what is left
        row = s.score_batch([set_corpus.WIDE_TIE_QUERY], 0.0, 10)[0]
        left = [k for k in (set_corpus.WIDE_TIE_QUERY + "%03d" % n for n in range(set_corpus.WIDE_FAMILY))
                if k not in set(removed)]
        assert [k for k, _ in row] == left[:10] and len(left) < set_corpus.WIDE_FAMILY // 2 + 1
    finally:
        s.dispose()
        oracle.close()
        for ix in members + [fresh]:
            ix.dispose()


# ---- 5. later stages --------------------------------------------------------------------------------------
def test_score_batch_sim_after_removal_equals_the_live_rows_index(lib):
    lib.use("a")
    fresh = lib.fresh("a")[0]
    qs = set_corpus.narrow_queries()[::3] + [b"E R", b"R E Q"]
    for metric, token_sort, min_sim in (("levenshtein", False, 0.0), ("osa", True, 0.3), ("partial", False, 0.5)):
        got = lib.set.score_batch_sim(qs, 0.3, 10, min_sim, metric, False, token_sort)
        want = fresh.score_batch_sim(qs, 0.3, 10, min_sim, metric, False, token_sort)
        assert [len(r) for r in got] == [len(r) for r in want] and sum(map(len, got)) > len(qs)
        same(got, want, f"sim by {metric}")  # strings, score bits and similarity bits


def test_self_join_rows_of_dead_keys_are_empty_and_no_dead_key_is_a_hit(lib):
    dead = set(lib.use("a"))
    fresh = lib.fresh("a")[0]
    kid = {fresh.key(k): k for k in range(fresh.num_keys())}
    want = fresh.self_join(0, None, 0.0, 10)
    empty = 0
    for first, count in ((0, 40), (2490, 30), (5980, 20)):  # across the members' boundaries
        got = lib.set.self_join(first, count, 0.0, 10)
        empty += sum(first + i in dead for i in range(count))
        for i, row in enumerate(got):
            g = first + i
            if g in dead:
                assert row == [], g
                continue
            assert not any(h in dead or h == g for h, _ in row), g
            w = want[kid[lib.names[g]]]
            assert [lib.names[h] for h, _ in row] == [fresh.key(k) for k, _ in w], g
            assert np.array_equal(np.array([x for _, x in row], dtype=np.float32).view(np.uint32),
                                  np.array([x for _, x in w], dtype=np.float32).view(np.uint32)), g
    assert empty >= 3
    # the device form: the same rows, dead ones with count 0
    first, count, stride = 2490, 30, 11
    d_n, d_k, d_s = dev(np.full(count, 9)), dev(np.zeros(count * stride)), dev(np.zeros(count * stride))
    lib.set.self_join_device(first, count, 0.0, 10, stride, d_n.data_ptr(), d_k.data_ptr(), d_s.data_ptr())
    host_rows = lib.set.self_join(first, count, 0.0, 10)
    assert host(d_n).tolist() == [len(r) for r in host_rows]
    assert all(host(d_n)[i] == 0 for i in range(count) if first + i in dead)


def test_dedup_gives_the_partition_of_the_live_keys(lib):
    dead = set(lib.use("a"))
    fresh = lib.fresh("a")[0]

    def partition(labels, key_of, skip=()):
        groups = {}
        for k, lab in enumerate(labels):
            if k not in skip:
                groups.setdefault(lab, []).append(key_of(k))
        return {frozenset(g) for g in groups.values()}

    L = _native.lib()
    for batch in (0, 64):
        labels = lib.set.dedup(0.3, 10, None, batch)
        assert all(labels[g] == g for g in dead)                       # dead labels are their own ids
        assert not any(labels[g] in dead for g in range(6000) if g not in dead)
        want_labels = fresh.dedup(0.3, 10, None, batch)
        want = partition(want_labels, fresh.key)
        assert partition(labels, lib.names.__getitem__, dead) == want and 1 < len(want) < fresh.num_keys()
        out = (C.c_uint32 * 6000)()
        assert L.dedupKeysSet(lib.set.set_id, 0.3, 10, 0, -1.0, batch, out) == len(want)  # live clusters only
