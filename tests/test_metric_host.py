"""CPU-side checks of the similarity's metrics and the matched term (no GPU compute): the new
exports and their argument checks, the model tests/metric_ref.py against hand-computed cases, and
the host routines of stringsearchlib_amd/csrc/ngs_sim.h (OSA and PARTIAL, one word and multi-word)
under ASan + UBSan against the model."""
import ctypes as C
import itertools
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import metric_cases
import metric_ref
import sim_ref
import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRIC_EXPORTS = ["ngsSimilarityDeviceM", "ngsRerankDeviceM", "scoreBatchSimM", "scoreBatchSimMW", "scoreBatchSimMU8",
                  "ngsReleaseTerms", "dedupKeysM", "ngsTerm"]
P = 0x1000  # a non-null "device pointer": the calls below fail before anything is read through it
HIP_INVALID_VALUE = 1


def test_header_declares_and_library_exports_metric_symbols():
    syms = _native.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    L = _native.lib()
    for s in METRIC_EXPORTS:
        assert s in syms, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"
    header = open(_native.HEADER).read()
    for name, value in (("NGS_SIM_LEVENSHTEIN", 0), ("NGS_SIM_OSA", 1), ("NGS_SIM_PARTIAL", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}u\b", header), name
    assert ssl.METRICS == {"levenshtein": 0, "osa": 1, "partial": 2} == metric_ref.METRICS
    assert ssl.NO_TERM == metric_ref.NO_TERM == 0xFFFFFFFF


def test_metric_argument_checks_without_gpu_work():
    L = _native.lib()
    words = (C.c_char_p * 1)(b"seulement")
    h = L.indexN(words, 1, 1, None)  # one word: an un-built handle, no GPU touched
    assert h
    res = C.POINTER(C.POINTER(C.c_char))()
    sc, sv, tv = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
    qs = (C.c_char_p * 2)(b"a", b"b")
    buf = (C.c_uint8 * 16)()
    try:
        for metric in (0, 1, 2):
            assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, P, P, metric, P, P, None) == -2
            assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, P, P, metric, P, None, None) == -2  # dTerms may be null
            assert L.ngsRerankDeviceM(h, P, P, 4, 8, P, P, P, P, P, metric, 0.5, None) == -2
            assert L.ngsRerankDeviceM(h, P, P, 4, 8, P, P, P, P, None, metric, 0.5, None) == -2
        # bad arguments answer before the handle is looked at: an unknown metric among them
        for bad in (3, 7, 0xFFFFFFFF):
            assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, P, P, bad, P, P, None) == -3
            assert L.ngsRerankDeviceM(h, P, P, 4, 8, P, P, P, P, P, bad, 0.5, None) == -3
            assert L.ngsSimilarityDeviceM(h + 1000, P, P, 4, 8, P, P, bad, P, P, None) == -3
        assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, None, P, 1, P, P, None) == -3  # null dCounts
        assert L.ngsSimilarityDeviceM(h, P, None, 4, 8, P, P, 1, P, P, None) == -3  # null offsets
        assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, P, None, 1, P, P, None) == -3  # null keys with records to read
        assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, P, P, 1, None, P, None) == -3  # null dSim
        assert L.ngsRerankDeviceM(h, P, P, 4, 8, None, P, P, P, P, 2, 0.5, None) == -3
        assert L.ngsRerankDeviceM(h, P, P, 4, 8, P, P, None, P, P, 2, 0.5, None) == -3  # null dScores
        assert L.ngsRerankDeviceM(h, P, P, 4, 4097, P, P, P, P, P, 2, 0.5, None) == -3  # stride above the cap
        assert L.ngsRerankDeviceM(h, P, P, 4, 4096, P, P, P, P, P, 2, 0.5, None) == -2
        assert L.ngsRerankDeviceM(h, P, P, 4, 8, P, P, P, P, P, 2, float("nan"), None) == -3
        # scoreBatchSimM on an un-built handle: 0, counts zeroed, outputs untouched
        for fn in (L.scoreBatchSimM, L.scoreBatchSimMU8):
            counts = (C.c_uint32 * 2)(7, 7)
            assert fn(h, qs, 2, 0.0, 10, 1, 0.5, counts, C.byref(res), C.byref(sc), C.byref(sv), C.byref(tv)) == 0
            assert list(counts) == [0, 0] and not res and not sc and not sv and not tv
        # ngsTerm on an un-built handle
        assert L.ngsTerm(h, 0, None, 0) == -2 and L.ngsTerm(h, 0, buf, 16) == -2
        # dedupKeysM: an unknown metric is a HIP invalid-value code, before the handle
        labels = (C.c_uint32 * 4)(9, 9, 9, 9)
        L.ngsLastError(1)
        assert L.dedupKeysM(h, 0.5, 10, 3, 0.5, 0, labels) == 0
        assert L.ngsLastError(1) == HIP_INVALID_VALUE and list(labels) == [9, 9, 9, 9]
        assert L.dedupKeysM(h, 0.5, 10, 1, 0.5, 0, labels) == 0  # un-built
        assert L.ngsLastError(1) == HIP_INVALID_VALUE
    finally:
        L.dispose(h)
    assert L.ngsSimilarityDeviceM(h + 1000, P, P, 4, 8, P, P, 1, P, P, None) == -1
    assert L.ngsRerankDeviceM(h + 1000, P, P, 4, 8, P, P, P, P, P, 2, 0.5, None) == -1
    assert L.ngsTerm(h + 1000, 0, None, 0) == -1
    counts = (C.c_uint32 * 2)(7, 7)
    assert L.scoreBatchSimM(h + 1000, qs, 2, 0.0, 10, 1, 0.5, counts, C.byref(res), C.byref(sc), C.byref(sv), None) == 0
    assert list(counts) == [0, 0]
    L.ngsReleaseTerms(None)
    with pytest.raises(ValueError):
        ssl.index._metric("damerau")
    with pytest.raises(ValueError):
        ssl.index._metric(3)
    assert [ssl.index._metric(x) for x in ("levenshtein", "osa", "partial", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]


def test_model_agrees_with_hand_computed_cases():
    assert metric_ref.osa(b"CA", b"AC") == 1
    assert metric_ref.osa(b"CA", b"ABC") == 3  # unrestricted Damerau gives 2: no substring is edited twice
    assert sim_ref.lev(b"CA", b"AC") == 2
    assert metric_ref.partial(b"ACME", b"XXACNEYY") == 1
    assert metric_ref.partial(b"ACME", b"ACME HOLDINGS INTERNATIONAL") == 0
    assert metric_ref.partial(b"ACME HOLDINGS INTERNATIONAL", b"ACME") == 23  # directional
    assert metric_ref.partial(b"", b"ABC") == 0 and metric_ref.partial(b"ABC", b"") == 3
    assert metric_ref.partial(b"ABC", b"XYZ") == 3  # the empty substring: d <= m
    assert metric_ref.osa(b"", b"ABC") == 3 and metric_ref.osa(b"ABCD", b"BADC") == 2
    s = metric_ref.sim_value
    assert s(1, 10, 10, metric_ref.OSA) == np.float32(1.0) - np.float32(1.0) / np.float32(10.0)
    assert s(1, 4, 8, metric_ref.PARTIAL) == np.float32(0.75) and s(0, 0, 5, metric_ref.PARTIAL) == np.float32(0.0)
    assert s(3, 0, 3, metric_ref.OSA) == np.float32(0.0)


def test_model_batch_rows_equal_the_cell_by_cell_dps():
    rng = random.Random(11)
    qs = [tuple(rng.choice(b"ABC") for _ in range(rng.randint(0, 24))) for _ in range(500)]
    ts = [tuple(rng.choice(b"ABC") for _ in range(rng.randint(0, 24))) for _ in range(500)]
    for q, t in metric_cases.swap_pairs(rng, 9, b"ABC", reps=5):
        qs.append(q)
        ts.append(t)
    for metric in (metric_ref.LEVENSHTEIN, metric_ref.OSA, metric_ref.PARTIAL):
        got = metric_ref.dist_batch(qs, ts, metric)
        assert [int(x) for x in got] == [metric_ref.dist(q, t, metric) for q, t in zip(qs, ts)], metric
    for q, t in list(zip(qs, ts))[:120]:
        assert metric_ref.partial(q, t) == metric_ref.partial_by_definition(q, t)
    # the tie rule: the smaller term id among equal similarities, whatever the order of the set
    ids = {tuple(b"ABX"): 5, tuple(b"ABY"): 2, tuple(b"Q"): 0}
    sims, best = metric_ref.record_sims([(b"abz", set(ids)), (b"*", set(ids)), (b"abz", None)], metric_ref.OSA, ids)
    assert best == [tuple(b"ABY"), None, None] and sims[1] == 1.0 and sims[2] == -1.0


PLANTED_M = (2, 3, 8, 33, 63, 64, 65, 127, 128, 129, 4096)


def _pairs():
    """(Q, T) pairs, already normalised: all over {A, B} of lengths 0..5 on both sides, 10,000 seeded random
    ones of lengths 1..80 over four letters, planted swap pairs and planted substring pairs."""
    short = [tuple(t) for n in range(6) for t in itertools.product(b"AB", repeat=n)]
    pairs = [(q, t) for q in short for t in short]
    rng = random.Random(0x05A)
    rs = lambda n: tuple(rng.choice(b"ACGT") for _ in range(n))
    pairs += [(rs(rng.randint(1, 80)), rs(rng.randint(1, 80))) for _ in range(10000)]
    swaps, subs = [], []
    for m in PLANTED_M:
        swaps += metric_cases.swap_pairs(rng, m, reps=1 if m == 4096 else 3)
        subs += metric_cases.substring_pairs(rng, m, reps=1 if m == 4096 else 3)
    return pairs, swaps, subs


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_host_metrics_under_sanitizers_match_the_model(tmp_path):
    """tests/sanitize/metric_driver.cpp (its own main, ngs_sim.h alone, g++ -fsanitize=address,undefined)
    against metric_ref: the distance and the fp32 bits of sim from the one-word and the multi-word routine of
    both metrics."""
    pairs, swaps, subs = _pairs()
    assert len(pairs) == 63 * 63 + 10000
    # the planted pairs tell the metrics apart, and reach the places the carries cross
    metric_cases.assert_not_vacuous(swaps, subs)
    diff = lambda q, t: [i for i in range(len(q)) if q[i] != t[i]]
    assert any(len(q) > 64 and {63, 64} <= set(diff(q, t)) for q, t in swaps)
    assert any(len(q) > 128 and {127, 128} <= set(diff(q, t)) for q, t in swaps)
    for m in PLANTED_M:
        mine = [(q, t) for q, t in swaps if len(q) == m]
        assert any({0, 1} <= set(diff(q, t)) for q, t in mine), m
        assert any({m - 2, m - 1} <= set(diff(q, t)) for q, t in mine), m
    pairs += swaps + subs

    exe = str(tmp_path / "metric_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "metric_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(pairs)))
        f.write(b"".join(struct.pack("<H", len(q)) + bytes(q) + struct.pack("<H", len(t)) + bytes(t) for q, t in pairs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip() == f"ok {len(pairs)}", p.stdout
    got = np.fromfile(dst, dtype="<u4").reshape(len(pairs), 8)

    qs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    want = np.zeros((len(pairs), 8), dtype=np.uint32)
    for col, metric in ((0, metric_ref.OSA), (4, metric_ref.PARTIAL)):
        d = metric_ref.dist_batch(qs, ts, metric)
        for i, di in enumerate(d):
            m, ln = len(qs[i]), len(ts[i])
            b = np.float32(metric_ref.sim_value(int(di), m, ln, metric)).view(np.uint32)
            want[i, col:col + 4] = (di, b, di, b) if m <= 64 else (0xFFFFFFFF, 0, di, b)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"pair {bad[0]} {pairs[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"

