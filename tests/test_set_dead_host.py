"""CPU-side checks of dead keys in index sets (no GPU compute): the new exports and their bindings, the
argument checks that answer before the GPU is touched, the numpy model of the row rule
(tests/dead_ref.py) on the planted cases, the host routine of stringsearchlib_amd/csrc/ngs_set.h in a
stand-alone program under ASan + UBSan against the model, a model of the over-fetch loop, and the
removal plans of the GPU tests against the oracle's ambiguity flag."""
import ctypes as C
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dead_cases
import dead_corpus
import dead_ref
import set_corpus
from stringsearchlib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # a non-null "device pointer": the calls below fail before anything is read through it
CASES = dead_cases.cases()
NEW = ("ngsDropDeadDevice", "ngsSetRemove", "ngsSetRestore", "ngsSetLiveKeys", "ngsSetDeadKeys", "ngsSetIsLive",
       "ngsSetDeadStats")


def test_header_declares_and_library_exports_dead_key_symbols():
    syms = _native.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    L = _native.lib()
    for s in NEW:
        assert s in syms, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"
    header = open(_native.HEADER).read()
    assert re.search(r"#define\s+NGS_SET_DEAD_STATS\s+3u\b", header)
    import stringsearchlib_amd as ssl
    assert "drop_dead_device" in ssl.__all__ and callable(ssl.drop_dead_device)
    for m in ("remove", "restore", "live_keys", "dead_keys", "is_live", "dead_stats"):
        assert hasattr(ssl.IndexSet, m), m


def test_the_model_sits_on_the_headers_constants():
    text = open(os.path.join(ROOT, "stringsearchlib_amd", "csrc", "ngs_set.h")).read()

    def const(name):
        return int(re.search(rf"constexpr uint32_t {name} = (\d+);", text).group(1))

    assert const("kSetDeadFetch0") == dead_ref.FETCH0 and const("kSetDeadFetchGrowth") == dead_ref.GROWTH
    assert const("kSetDeadFastLimit") == dead_ref.FAST_LIMIT and const("kSetDeadFetchMin") == dead_ref.FETCH_MIN
    common = open(os.path.join(ROOT, "stringsearchlib_amd", "csrc", "ngs_common.h")).read()
    assert int(re.search(r"constexpr uint32_t kWaveMaxLimit = (\d+);", common).group(1)) == dead_ref.FAST_LIMIT
    assert [dead_ref.first_fetch(10 ** 6, L) for L in (1, 10, 100, 112, 113, 128, 1000, dead_ref.LIMIT_ALL)] == \
        [127, 118, 28, 16, 113, 128, 1000, 10 ** 6]
    assert const("kSetOneWaveRecords") == dead_cases.ONE_WAVE and const("kSetThreads") == dead_cases.THREADS
    assert dead_ref.GROWTH >= 2  # the loop ends


def test_drop_dead_argument_checks_without_gpu_work():
    """Integers stand in for the device pointers: every call answers -3 before any HIP call."""
    L = _native.lib()

    def call(c=P, k=P, s=P, n=4, stride=8, dead=P, n_keys=40, limit=0, short=P):
        return L.ngsDropDeadDevice(c, k, s, n, stride, dead, n_keys, limit, short, None)

    assert call(c=None) == -3 and call(c=None, n=0) == -3
    assert call(k=None) == -3 and call(s=None) == -3
    assert call(dead=None) == -3 and call(dead=None, n=0) == -3
    assert call(n=0x80000000) == -3  # more rows than a grid holds
    # what is allowed answers 0 without a launch when there are no rows
    assert call(n=0) == 0 and call(n=0, k=None, s=None, stride=0) == 0
    assert call(n=0, dead=None, n_keys=0, short=None) == 0


def test_dead_key_calls_on_unknown_sets():
    L = _native.lib()
    unknown = 12345
    ids = (C.c_uint32 * 2)(0, 1)
    out = (C.c_uint32 * 2)(7, 7)
    stats = (C.c_uint64 * 3)(7, 7, 7)
    assert L.ngsSetRemove(unknown, ids, 2) == -1 and L.ngsSetRestore(unknown, ids, 2) == -1
    assert L.ngsSetRemove(unknown, None, 0) == -1
    assert L.ngsSetLiveKeys(unknown) == 0 and L.ngsSetDeadKeys(unknown, out, 2) == 0 and list(out) == [7, 7]
    assert L.ngsSetIsLive(unknown, 0) == -1
    assert L.ngsSetDeadStats(unknown, stats, 3) == -1 and list(stats) == [7, 7, 7]


# ---- the model on the planted cases ---------------------------------------------------------------
def brute(block, limit):
    """The row rule written the long way round: by key id sets instead of mask words."""
    dead = {k for k in range(block["n_keys"]) if (int(block["dead"][k >> 5]) >> (k & 31)) & 1}
    L = limit or dead_ref.LIMIT_ALL
    counts, rows, short = [], [], 0
    for i in range(block["n"]):
        c = min(int(block["counts"][i]), block["stride"])
        recs = [(int(block["keys"][i * block["stride"] + r]), int(block["scores"][i * block["stride"] + r]))
                for r in range(c)]
        live = [x for x in recs if x[0] not in dead]
        if c == block["stride"] and len(live) < L:
            short += 1
        rows.append(live[:L])
        counts.append(len(rows[-1]))
    return counts, rows, short


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_equals_brute_force_on_the_cases(case):
    name, block, limits = case
    for limit in limits:
        counts, rows, short = dead_ref.drop(block, limit)
        bc, br, bs = brute(block, limit)
        assert counts.tolist() == bc and rows == br and short == bs, (name, limit)


def test_cases_hold_what_they_are_meant_to():
    by = {c[0]: c[1] for c in CASES}
    for side, stride in (("wave", 256), ("group", 1150)):
        for pat in ("all", "none", "first", "last", "alternate", "run"):
            b = by[f"{side}-{pat}"]
            assert b["stride"] == stride and b["counts"].tolist() == list(dead_cases.COUNTS)
        assert (by[f"{side}-all"]["stride"] <= dead_cases.ONE_WAVE) == (side == "wave")
        assert dead_ref.drop(by[f"{side}-all"], 0)[0].tolist() == [0] * len(dead_cases.COUNTS)
        none = dead_ref.drop(by[f"{side}-none"], 0)[0].tolist()
        assert none == [min(c, stride) for c in dead_cases.COUNTS]
        first = dead_ref.drop(by[f"{side}-first"], 0)[0].tolist()
        assert first == [max(0, min(c, stride) - 1) for c in dead_cases.COUNTS]
        # the dead run lies across the first chunk boundary of the launch
        chunk = 64 if side == "wave" else dead_cases.THREADS
        b, i = by[f"{side}-run"], len(dead_cases.COUNTS) - 1
        row = b["keys"][i * stride:(i + 1) * stride]
        assert dead_ref.is_dead(b, int(row[chunk - 1])) and dead_ref.is_dead(b, int(row[chunk]))
        assert not dead_ref.is_dead(b, int(row[chunk - 7])) and not dead_ref.is_dead(b, int(row[chunk + 5]))
    # rows above the stride are read as the stride, and some are short
    assert dead_ref.drop(by["wave-alternate"], 300)[2] >= 3 and dead_ref.drop(by["wave-none"], 256)[2] == 0
    assert dead_ref.drop(by["group-random"], 700)[2] > 0
    e = by["edges"]
    assert [dead_ref.is_dead(e, k) for k in (30, 31, 32, 33, 62, 63, 64, 65)] == [False, True, False, False, False,
                                                                                 False, True, False]
    assert (int(e["dead"][-1]) >> (4095 & 31)) & 1 and not dead_ref.is_dead(e, 4095)  # a set bit past n_keys
    assert dead_ref.drop(e, 0)[1][0][-6:] == [(k, int(e["scores"][10 + j])) for j, k in
                                              enumerate((dead_cases.N_KEYS, dead_cases.N_KEYS + 3, 4095, 4096,
                                                         0x7FFFFFFF, 0xFFFFFFFF))]
    assert by["no-mask"]["dead"] is None and dead_ref.drop(by["no-mask"], 0)[0].tolist() == [3, 70, 0]
    assert dead_ref.drop(by["stride-0"], 0)[0].tolist() == [0, 0] and dead_ref.drop(by["stride-0"], 3)[2] == 2


# ---- ngs_set.h under sanitizers ----------------------------------------------------------------------
def record(block, limit):
    """One block as tests/sanitize/dead_driver.cpp reads it."""
    words = 0 if block["dead"] is None else len(block["dead"])
    body = [struct.pack("<5I", block["n"], block["stride"], block["n_keys"], limit, words),
            block["counts"].astype("<u4").tobytes(), block["keys"].astype("<u4").tobytes(),
            block["scores"].astype("<u4").tobytes()]
    if words:
        body.append(block["dead"].astype("<u4").tobytes())
    return b"".join(body)


def flat(counts, rows, short):
    out = [counts.astype("<u4"), np.array([short], dtype="<u4")]
    for r in rows:
        out += [np.array([k for k, _ in r], dtype="<u4"), np.array([b for _, b in r], dtype="<u4")]
    return np.concatenate(out)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_host_drop_routine_under_sanitizers_matches_model(tmp_path):
    """tests/sanitize/dead_driver.cpp (its own main, ngs_set.h alone, g++ -fsanitize=address,undefined):
    drop_dead_row on every case at every limit and on 300 random small cases, every row and the mask in
    buffers of their exact size; the output must be the model's."""
    exe = str(tmp_path / "dead_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "dead_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    rng = random.Random(0xDEAD2)
    runs = [(block, limit) for _, block, limits in CASES for limit in limits]
    runs += [dead_cases.random_small(rng) for _ in range(300)]
    records = [record(b, limit) for b, limit in runs]
    want = [flat(*dead_ref.drop(b, limit)) for b, limit in runs]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip() == f"ok {len(records)}", p.stdout
    got = np.frombuffer(open(dst, "rb").read(), dtype="<u4")
    exp = np.concatenate(want)
    assert len(got) == len(exp)
    assert (got == exp).all(), np.flatnonzero(got != exp)[:5]


# ---- the over-fetch loop -----------------------------------------------------------------------------
def test_over_fetch_loop_gives_the_first_live_records_and_stops_at_the_dead_count():
    """Searching at L + E, dropping, and fetching again while short gives the first L live records of
    the member's hit list, whatever the hits and the dead set; the last over-fetch is at most d."""
    rng = random.Random(0xFE7C)
    grew = exact = 0
    for t in range(600):
        n_keys = rng.choice((1, 5, 64, 65, 300, 2000))
        hits = rng.sample(range(n_keys), rng.choice((0, n_keys // 3, n_keys)))
        shape = rng.choice(("none", "few", "head", "most", "all"))
        if shape == "head":  # the best hits are the dead ones: what makes a row short
            dead = set(hits[:rng.randrange(0, len(hits) + 1)])
        else:
            frac = {"none": 0.0, "few": 0.05, "most": 0.9, "all": 1.0}[shape]
            dead = {k for k in range(n_keys) if rng.random() < frac}
        limit = rng.choice((0, 1, 2, 10, 63, 64, 100, 112, 113, 200))
        row, used = dead_ref.over_fetch(hits, dead, n_keys, limit)
        L = limit or dead_ref.LIMIT_ALL
        assert row == [k for k in hits if k not in dead][:L], t
        d = len(dead)
        assert (used == []) == (d == 0), t
        if used:
            assert used[0] == dead_ref.first_fetch(d, L) and used[-1] <= d, t
            assert all(b == min(d, a * dead_ref.GROWTH) and b > a for a, b in zip(used, used[1:])), t
            grew += len(used) > 1
            exact += used[-1] == d
    assert grew > 20 and exact > 100  # the loop was exercised: it grew, and it reached E = d


# ---- the plans of the GPU tests against the oracle ----------------------------------------------------
@pytest.mark.parametrize("name", dead_corpus.PLANS)
def test_oracle_flags_none_of_the_narrow_queries_over_the_live_rows(name):
    """tests/test_gpu_set_dead.py compares every narrow query with the oracle over the rows a plan
    leaves, none skipped: the allowance for ambiguous answers is zero."""
    from oracle_py import OracleIndex
    words, weights, cuts = set_corpus.narrow()
    removed = dead_corpus.plan(name)
    masters = words[::set_corpus.ROW]
    assert len(set(removed)) == len(removed) and set(removed) <= set(masters)
    w, wt = dead_corpus.live_rows(words, weights, removed)
    oi = OracleIndex(w, set_corpus.ROW, wt)
    try:
        assert oi.n_keys() == len(masters) - len(removed)
        qs = set_corpus.narrow_queries()
        for thr in set_corpus.THRESHOLDS:
            for limit in set_corpus.LIMITS:
                assert not [q for q in qs if oi.score_amb(q, thr, limit)[1]], (name, thr, limit)
    finally:
        oi.close()


def test_plans_hold_what_they_are_meant_to():
    words, _, cuts = set_corpus.narrow()
    masters = words[::set_corpus.ROW]
    fam = dead_corpus.family()
    assert set(fam) <= set(masters) and [masters.index(k) for k in fam] == sorted(masters.index(k) for k in fam)
    assert len(dead_corpus.plan("a")) == 600
    assert dead_corpus.plan("b") == tuple(fam[::2])
    c = dead_corpus.plan("c")
    assert len(c) >= 24 and set_corpus.TIE_QUERY + b"299" in c and masters[0] in c
    assert dead_corpus.plan("d") == (masters[0], masters[1]) and cuts[1] == 2
    # (e): the second member's family keys all die, and they are more than the first over-fetch at limit 10
    e = set(dead_corpus.plan("e"))
    second = [k for k in masters[cuts[1]:cuts[2]] if k in set(fam)]
    assert len(e) == 150 and set(second) <= e and len(second) > dead_ref.first_fetch(len(second), 10) == 118
