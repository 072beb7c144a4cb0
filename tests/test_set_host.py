"""CPU-side checks of index sets (no GPU compute): the new exports and their bindings, the argument
checks that answer before any handle or the GPU is touched, the set calls on unknown ids, the numpy
model of the merge (tests/set_ref.py) against a brute-force sort, and the host routine of
stringsearchlib_amd/csrc/ngs_set.h in a stand-alone program under ASan + UBSan against the model."""
import ctypes as C
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import set_cases
import set_ref
from stringsearchlib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # a non-null "device pointer": the calls below fail before anything is read through it
HIP_INVALID_VALUE = 1
CASES = set_cases.cases()
NEW = ("ngsKeyLengthsDevice", "ngsMergeResultsDevice", "ngsSetCreate", "ngsSetAdd", "ngsSetDispose", "ngsSetParts",
       "ngsSetNumKeys", "ngsSetLocate", "ngsSetSearchDevice", "scoreBatchSet", "scoreBatchSetW", "scoreBatchSetU8")


def test_header_declares_and_library_exports_set_symbols():
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
    assert re.search(r"#define\s+NGS_SET_MAX_PARTS\s+16u\b", header)
    assert "ngs_merge_part" in header and set_cases.MAX_PARTS == 16
    assert C.sizeof(_native.MergePart) == 48  # 16 parts x 48 bytes travel in the kernel arguments
    import stringsearchlib_amd as ssl
    assert "IndexSet" in ssl.__all__ and "merge_results_device" in ssl.__all__
    assert callable(ssl.merge_results_device) and callable(ssl.StringIndex.key_lengths_device)
    for m in ("add", "append", "parts", "num_keys", "locate", "key", "score_batch", "search_device", "dispose"):
        assert hasattr(ssl.IndexSet, m), m
    assert ssl.METRICS == {"levenshtein": 0, "osa": 1, "partial": 2}


def _parts(*rows):
    arr = (_native.MergePart * max(1, len(rows)))()
    for a, r in zip(arr, rows):
        a.dCounts, a.dKeys, a.dScores, a.stride, a.keyBase, a.dKeyLen, a.nKeys = r
    return arr


def test_merge_results_argument_checks_without_gpu_work():
    """Integers stand in for the device pointers: every call answers -3 before any HIP call."""
    L = _native.lib()
    good = (P, P, P, 8, 0, P, 5)

    def call(parts, n_parts, n=4, limit=0, stride=16, c=P, k=P, s=P):
        return L.ngsMergeResultsDevice(parts, n_parts, n, limit, stride, c, k, s, None)

    two = _parts(good, good)
    assert call(None, 2) == -3
    assert call(two, 0) == -3 and call(_parts(*[good] * 17), 17, stride=200) == -3
    assert call(two, 2, n=0x80000000) == -3 and call(two, 2, n=0xFFFFFFFF) == -3  # more queries than a grid holds
    assert call(two, 2, c=None) == -3 and call(two, 2, k=None) == -3 and call(two, 2, s=None) == -3
    assert call(_parts(good, (None, P, P, 8, 0, P, 5)), 2) == -3      # a part without counts
    assert call(_parts(good, (P, None, P, 8, 0, P, 5)), 2) == -3      # records and no keys
    assert call(_parts(good, (P, P, None, 8, 0, P, 5)), 2) == -3      # records and no scores
    assert call(_parts(good, (P, P, P, 8, 0, None, 5)), 2) == -3      # keys and no lengths
    assert call(two, 2, stride=15) == -3 and call(two, 2, limit=16, stride=15) == -3
    assert call(two, 2, limit=9, stride=8) == -3
    # the sum of the strides in 64 bits: 2 x 2^31 does not wrap to 0
    wide = (P, P, P, 0x80000000, 0, P, 5)
    assert call(_parts(wide, wide), 2, limit=0, stride=100) == -3


def test_key_lengths_argument_checks_without_gpu_work():
    L = _native.lib()
    unknown = 0x7FFF0000
    assert L.ngsKeyLengthsDevice(unknown, 0, 4, None, None) == -3     # before the handle
    assert L.ngsKeyLengthsDevice(unknown, 0, 4, P, None) == -1
    assert L.ngsKeyLengthsDevice(unknown, 0, 0, None, None) == -1
    words = (C.c_char_p * 1)(b"seulement")
    h = L.indexN(words, 1, 1, None)  # one word: an un-built handle, no GPU touched
    assert h
    try:
        assert L.ngsKeyLengthsDevice(h, 0, 4, None, None) == -3
        assert L.ngsKeyLengthsDevice(h, 0, 0, None, None) == -2
    finally:
        L.dispose(h)


def test_set_calls_on_unknown_ids_and_bad_members():
    L = _native.lib()
    words = (C.c_char_p * 1)(b"seulement")
    h = L.indexN(words, 1, 1, None)  # un-built handles of two widths, no GPU touched
    w0 = (C.c_uint32 * 10)(*map(ord, "seulement"), 0)
    wide = (_native.W * 1)(C.cast(w0, _native.W))
    hw = L.indexW(wide, 1, 1, None, 2)
    assert h and hw

    def create_fails(handles, n=None):
        arr = (C.c_uint32 * max(1, len(handles)))(*handles)
        L.ngsLastError(1)
        assert L.ngsSetCreate(arr, len(handles) if n is None else n) == 0
        assert L.ngsLastError(1) == HIP_INVALID_VALUE

    try:
        create_fails([h + hw + 1000])           # an unknown handle
        create_fails([h], n=0)
        create_fails([h] * 17)
        create_fails([h, hw])                   # two widths
        create_fails([h])                       # not built
        L.ngsLastError(1)
        assert L.ngsSetCreate(None, 1) == 0 and L.ngsLastError(1) == HIP_INVALID_VALUE
        unknown = 12345
        hh, kk = C.c_uint32(7), C.c_uint32(7)
        assert L.ngsSetParts(unknown) == -1 and L.ngsSetNumKeys(unknown) == 0
        assert L.ngsSetLocate(unknown, 0, C.byref(hh), C.byref(kk)) == -1 and (hh.value, kk.value) == (7, 7)
        assert L.ngsSetAdd(unknown, h) == -1
        assert L.ngsSetSearchDevice(unknown, P, P, 1, 0.0, 10, 10, P, P, P, None) == -1
        L.ngsSetDispose(unknown)  # nothing to do
        counts = (C.c_uint32 * 2)(9, 9)
        keys = (C.c_uint32 * 20)()
        scores = (C.c_float * 20)()
        qs = (C.c_char_p * 2)(b"a", b"b")
        for fn, q in ((L.scoreBatchSet, qs), (L.scoreBatchSetU8, qs), (L.scoreBatchSetW, C.cast(qs, C.POINTER(_native.W)))):
            counts[0] = counts[1] = 9
            L.ngsLastError(1)
            assert fn(unknown, q, 2, 0.0, 10, 10, counts, keys, scores) == 0
            assert L.ngsLastError(1) == HIP_INVALID_VALUE and list(counts) == [0, 0]
        # set ids are not handles: nothing above took or freed an index handle
        assert L.ngsCharSize(h) == 1 and L.ngsCharSize(hw) == 4
    finally:
        L.dispose(h)
        L.disposeW(hw)


# ---- the model against a brute-force sort -----------------------------------------------------------
def _same(a, b):
    return (a[0] == b[0]).all() and a[1] == b[1]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_equals_brute_force_on_the_cases(case):
    name, parts, n, limits = case
    for limit in limits:
        got, want = set_ref.merge(parts, n, limit), set_ref.merge_brute(parts, n, limit)
        assert _same(got, want), (name, limit)
        total = [sum(min(int(p["counts"][i]), p["stride"]) for p in parts) for i in range(n)]
        assert got[0].tolist() == [min(t, limit or set_ref.LIMIT_ALL) for t in total]
        assert max(got[0]) <= set_ref.min_stride(parts, limit)
    # every row of every part is in merge order (the kernel's precondition): a part alone merges to itself
    for p in parts:
        alone = set_ref.merge([p], n, 0)[1]
        for i in range(n):
            c = min(int(p["counts"][i]), p["stride"])
            k = (p["keys"][i * p["stride"]:i * p["stride"] + c] + np.uint32(p["base"])).tolist()
            assert [g for g, _ in alone[i]] == k, name


def test_cases_hold_what_they_are_meant_to():
    by = {c[0]: c for c in CASES}
    assert any(int(c) > 7 for c in by["one-part"][1][0]["counts"]) and by["one-part"][1][0]["base"]
    assert [p["stride"] for p in by["uneven"][1]] == [1, 7, 100]
    assert len(by["sixteen"][1]) == 16 and {63, 64, 65, 80, 81} <= set(by["sixteen"][3])
    w = set_cases.ONE_WAVE // 4
    assert {0, 4096, w - 1, w, w + 1} <= set(by["large"][3])
    rows = [sum(min(int(p["counts"][i]), 3000) for p in by["lds-edge"][1]) for i in range(4)]
    assert rows == [set_cases.LDS - 1, set_cases.LDS, set_cases.LDS + 1, 12000]
    assert any((p["keys"][:5] >= len(p["lens"])).any() for p in by["ids-past"][1])
    seen = set(np.concatenate([p["scores"] for p in by["score-bits"][1]]).tolist())
    assert set(set_cases.ODD) <= seen
    # the tie class spans all parts and the limits fall inside it
    c, rows = set_ref.merge(by["tie-span"][1], 4, 10)
    assert len({b for _, b in rows[0]}) == 1 and {g // 12 for g, _ in rows[0]} == {0, 1}


def test_model_equals_brute_force_on_random_small_cases():
    rng = random.Random(0x5E75)
    for t in range(200):
        parts, n, limit = set_cases.random_small(rng)
        assert _same(set_ref.merge(parts, n, limit), set_ref.merge_brute(parts, n, limit)), t


def test_order_bits_is_the_floats_order():
    vals = np.array([-np.inf, -1.0, -1e-30, -0.0, 0.0, 1e-45, 1e-30, 0.25, 100.0, np.inf], dtype=np.float32)
    img = set_ref.order_bits(vals.view(np.uint32)).tolist()
    assert img == sorted(img) and len(set(img)) == len(img)


def test_oracle_flags_none_of_the_gpu_tests_queries():
    """tests/test_gpu_set.py compares every query of its narrow batch with the oracle, none skipped: the
    oracle's answer must not depend on the reference's map order for any of them, and the batch holds
    what it is meant to."""
    import set_corpus
    from oracle_py import OracleIndex
    words, weights, cuts = set_corpus.narrow()
    qs = set_corpus.narrow_queries()
    oi = OracleIndex(words, set_corpus.ROW, weights)
    assert oi.n_keys() == 6000 and 180 <= len(qs) <= 220 and cuts[1] - cuts[0] == 2
    for thr in set_corpus.THRESHOLDS:
        for limit in set_corpus.LIMITS:
            assert not [q for q in qs if oi.score_amb(q, thr, limit)[1]], (thr, limit)
    ties = oi.score(set_corpus.TIE_QUERY, 0.0, 0)
    assert sum(1 for _, s in ties if s == ties[0][1]) == set_corpus.FAMILY
    oi.close()


# ---- ngs_set.h under sanitizers ----------------------------------------------------------------------
def _build_driver(tmp_path):
    exe = str(tmp_path / "set_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "set_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def record(parts, n, limit, out_stride):
    """One merge as tests/sanitize/set_driver.cpp reads it."""
    u32 = lambda *v: struct.pack(f"<{len(v)}I", *v)
    body = [u32(len(parts), n, limit, out_stride)]
    for p in parts:
        lens = np.asarray(p["lens"], dtype="<u4")
        body += [u32(p["stride"], p["base"], len(lens)), p["counts"].astype("<u4").tobytes(),
                 p["keys"].astype("<u4").tobytes(), p["scores"].astype("<u4").tobytes(), lens.tobytes()]
    return b"".join(body)


def flat(counts, rows):
    out = [counts.astype("<u4")]
    for r in rows:
        out += [np.array([g for g, _ in r], dtype="<u4"), np.array([b for _, b in r], dtype="<u4")]
    return np.concatenate(out)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_host_merge_routine_under_sanitizers_matches_model(tmp_path):
    """tests/sanitize/set_driver.cpp (its own main, ngs_set.h alone, g++ -fsanitize=address,undefined):
    merge_rows on every case at every limit, and on 200 random small cases, into a block of exactly the
    least stride; the output must be the model's."""
    exe = _build_driver(tmp_path)
    records, want = [], []
    rng = random.Random(0x5E76)
    runs = [(parts, n, limit) for _, parts, n, limits in CASES for limit in limits]
    runs += [set_cases.random_small(rng) for _ in range(200)]
    for parts, n, limit in runs:
        records.append(record(parts, n, limit, set_ref.min_stride(parts, limit)))
        want.append(flat(*set_ref.merge(parts, n, limit)))
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
