"""CPU-side checks of the token sort (no GPU compute): the new export, the flag and their argument
checks, the model tests/token_ref.py on hand cases, and the host routine of
stringsearchlib_amd/csrc/ngs_token.h under ASan + UBSan against the model."""
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

import metric_ref
import sim_ref
import token_ref
import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # a non-null "device pointer": the calls below fail before anything is read through it
HIP_INVALID_VALUE = 1
FLAG = 0x100


def test_header_declares_and_library_exports_the_token_sort():
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert "ngsTokenSortDevice" in _native.declared_symbols()
    assert "ngsTokenSortDevice" in set(re.findall(r" T (\w+)$", out, re.M))
    assert _native.lib().ngsTokenSortDevice.argtypes is not None
    assert re.search(r"#define\s+NGS_SIM_TOKEN_SORT\s+0x100u\b", open(_native.HEADER).read())
    assert ssl.index.TOKEN_SORT == token_ref.TOKEN_SORT == FLAG
    assert ssl.METRICS == {"levenshtein": 0, "osa": 1, "partial": 2}
    m = ssl.index._metric
    assert [m(x) for x in (0x100, 0x101, 0x102, "osa")] == [0x100, 0x101, 0x102, 1]
    assert [m(x, True) for x in ("levenshtein", "osa", "partial", 2, 0x101)] == [0x100, 0x101, 0x102, 0x102, 0x101]
    for bad in ("jaro", 3, 0x103, 0x104, 0x200):
        with pytest.raises(ValueError):
            m(bad)
    for cls in (ssl.StringIndex, ssl.WideStringIndex, ssl.Utf8StringIndex):
        for name in ("score_batch_sim", "dedup", "similarity_device", "rerank_device"):
            assert "token_sort" in getattr(cls, name).__code__.co_varnames, (cls, name)
        assert callable(cls.token_sort_device)


def test_flag_argument_checks_without_gpu_work():
    L = _native.lib()
    words = (C.c_char_p * 1)(b"seulement")
    h = L.indexN(words, 1, 1, None)  # one word: an un-built handle, no GPU touched
    assert h
    res = C.POINTER(C.POINTER(C.c_char))()
    sc, sv, tv = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
    qs = (C.c_char_p * 2)(b"a", b"b")
    try:
        for metric in (0x100, 0x101, 0x102):  # -2 where 0..2 answer -2
            assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, P, P, metric, P, P, None) == -2
            assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, P, P, metric, P, None, None) == -2
            assert L.ngsRerankDeviceM(h, P, P, 4, 8, P, P, P, P, P, metric, 0.5, None) == -2
            counts = (C.c_uint32 * 2)(7, 7)
            L.ngsLastError(1)
            assert L.scoreBatchSimM(h, qs, 2, 0.0, 10, metric, 0.5, counts, C.byref(res), C.byref(sc), C.byref(sv),
                                    C.byref(tv)) == 0
            assert list(counts) == [0, 0] and not res and L.ngsLastError(1) == 0  # un-built, not a bad metric
        for bad in (0x103, 0x104, 0x200, 3, 7, 0xFFFFFFFF):  # unknown: before the handle is looked at
            assert L.ngsSimilarityDeviceM(h, P, P, 4, 8, P, P, bad, P, P, None) == -3
            assert L.ngsRerankDeviceM(h, P, P, 4, 8, P, P, P, P, P, bad, 0.5, None) == -3
            assert L.ngsSimilarityDeviceM(h + 1000, P, P, 4, 8, P, P, bad, P, P, None) == -3
            counts = (C.c_uint32 * 2)(7, 7)
            L.ngsLastError(1)
            assert L.scoreBatchSimM(h, qs, 2, 0.0, 10, bad, 0.5, counts, C.byref(res), C.byref(sc), C.byref(sv), None) == 0
            assert L.ngsLastError(1) in (0, HIP_INVALID_VALUE) and list(counts) == [0, 0]
            labels = (C.c_uint32 * 4)(9, 9, 9, 9)
            assert L.dedupKeysM(h, 0.5, 10, bad, 0.5, 0, labels) == 0
            assert L.ngsLastError(1) == HIP_INVALID_VALUE and list(labels) == [9, 9, 9, 9]
        # ngsTokenSortDevice: -3, then -1, then -2
        assert L.ngsTokenSortDevice(h, P, None, 4, P, None) == -3
        assert L.ngsTokenSortDevice(h, None, P, 4, P, None) == -3
        assert L.ngsTokenSortDevice(h, P, P, 4, None, None) == -3
        assert L.ngsTokenSortDevice(h + 1000, P, None, 0, P, None) == -3  # before the handle
        assert L.ngsTokenSortDevice(h + 1000, P, P, 4, P, None) == -1
        assert L.ngsTokenSortDevice(h + 1000, None, P, 0, None, None) == -1  # n = 0: the pointers may be null
        assert L.ngsTokenSortDevice(h, P, P, 4, P, None) == -2
        assert L.ngsTokenSortDevice(h, None, P, 0, None, None) == -2
    finally:
        L.dispose(h)
    assert L.ngsTokenSortDevice(h, P, P, 4, P, None) == -1


def ts(s, **kw):
    return bytes(token_ref.token_sort(s, **kw))


def test_model_on_hand_cases():
    assert ts(b"JOHN SMITH") == ts(b"SMITH JOHN") == b"JOHN SMITH"
    assert ts(b"ACME HOLDINGS") == ts(b"HOLDINGS ACME") == b"ACME HOLDINGS"
    assert ts(b"SMITH, JOHN") == b"JOHN SMITH "  # the comma is a separator: the length stays
    assert ts(b"A  B") == b"A B " and ts(b"B A") == b"A B"
    assert token_ref.sorted_query(b"A  B") == token_ref.sorted_query(b"B A") == tuple(b"A B")
    assert ts(b"A  B", stored=True) == b"A B" and ts(b"  B   A ", stored=True) == b"A B"
    # raw characters are written, the normalised ones compared; equal tokens keep their order
    assert ts(b"smith John") == b"John smith" and ts(b"ab AB Ab aB") == b"ab AB Ab aB"
    assert ts(b"ABC AB A") == b"A AB ABC"  # a proper prefix first
    assert ts(b"b\x80a") == b"a b" and ts(b"\xffz\xfea") == b"a z "  # bytes >= 0x80 are separators by default
    # the wildcard-adjacent strings
    assert ts(b"") == b"" and ts(b"*") == b"*" and ts(b"   ") == b"   "
    assert ts(b" *") == b"  " and ts(b" *", valid=sim_ref.DEFAULT_VALID + b"*") == b"* "
    assert sim_ref.is_wildcard(ts(b"")) and sim_ref.is_wildcard(ts(b"*"))
    assert not sim_ref.is_wildcard(ts(b"   ")) and not sim_ref.is_wildcard(ts(b" *"))
    assert token_ref.sorted_query(b"   ") == token_ref.sorted_query(b" *") == ()
    # a validChar set with a but not A: 'A' is a separator, and what k_sim normalises is the sorted normalised string
    v = bytes(c for c in sim_ref.DEFAULT_VALID if c != ord("A"))
    assert ts(b"zAa b", valid=v) == b"a b z" and token_ref.sorted_query(b"zAa b", v) == tuple(b"A B Z")
    # wide: characters from 128 are kept, values above 0x10FFFF separate
    assert token_ref.token_sort([0x65E5, 0x110000, 0xE9, 32, 65], wide=True) == (65, 32, 0xE9, 32, 0x65E5)
    # the 4,096 rule: the span between the first and the last kept character
    s4096 = b" " + b"B" * 2047 + b" " + b"A" * 2048 + b"  "
    assert ts(s4096) == b"A" * 2048 + b" " + b"B" * 2047 + b"   "
    s4097 = b" " + b"B" * 2048 + b" " + b"A" * 2048 + b"  "
    assert ts(s4097) == s4097 and ts(s4097[1:-2], stored=True) == s4097[1:-2]
    many = b"B A " * 1023 + b"B A"  # 2,048 tokens in 4,095 characters
    assert len(many) == 4095 and ts(many) == b"A " * 1024 + b"B " * 1023 + b"B"
    # the record similarity: the reordered name is the name
    one = np.float32(1.0)
    for metric in (metric_ref.LEVENSHTEIN, metric_ref.OSA, metric_ref.PARTIAL):
        assert token_ref.sorted_sim(b"smith, john", b"JOHN SMITH", metric) == one
    assert token_ref.plain_sim(b"smith john", b"JOHN SMITH", metric_ref.LEVENSHTEIN) < np.float32(0.3)
    # L' < L changes the divisor: "A  B" (L = 4) against "B A" is 1.0 sorted, d = 3 of 4 plain
    assert token_ref.sorted_sim(b"B A", b"A  B", metric_ref.LEVENSHTEIN) == one
    # the matched term is the term as indexed, the smaller id among equal sorted forms
    ids = {tuple(b"B A"): 4, tuple(b"A B"): 7, tuple(b"Q"): 0}
    sims, best = token_ref.record_sims([(b"a b", set(ids)), (b"*", set(ids)), (b"a b", None)], metric_ref.OSA, ids)
    assert best == [tuple(b"B A"), None, None] and list(sims) == [1.0, 1.0, -1.0]


def test_planted_reorder_pairs_need_the_flag():
    pairs = token_ref.reorder_pairs(random.Random(0x7C), 40)
    token_ref.assert_reorder_matters(pairs)


def _strings():
    """(cs, stored, characters): every string over {A, B, blank} up to length 7 in both forms, 10,000 seeded
    random ones (narrow and wide, separators of every kind), spans of 4,096 and 4,097."""
    out = []
    for n in range(8):
        for t in itertools.product(b"AB ", repeat=n):
            out.append((1, n % 2, list(t)))
            out.append((1, 1 - n % 2, list(t)))
    rng = random.Random(0x7D)
    narrow = list(b"abAB") * 3 + [32, 9, 13, ord(","), ord("*"), 0, 0x80, 0xFF, ord("z"), ord("0")]
    wide = list(b"abAB") * 3 + [32, 10, ord("-"), 0x110000, 0xFFFFFFFF, 0xE9, 0x65E5, 0x1F600, 0x80, ord("Z")]
    for i in range(10000):
        cs = 4 if i % 2 else 1
        out.append((cs, 1 if i % 5 == 0 else 0, [rng.choice(wide if cs == 4 else narrow) for _ in range(rng.randint(0, 40))]))
    for cs in (1, 4):
        for stored in (0, 1):
            for span in (4096, 4097):
                body = [rng.choice(b"ab AB") for _ in range(span - 2)]
                out.append((cs, stored, [32, 32] + [ord("c")] + body + [ord("C")] + [32]))
            out.append((cs, stored, list(b"B A " * 1023 + b"B A")))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_host_token_sort_under_sanitizers_matches_the_model(tmp_path):
    """tests/sanitize/token_driver.cpp (its own main, ngs_token.h alone, g++ -fsanitize=address,undefined): the
    host routine out of place, in place and against the driver's brute-force sort; its output against token_ref."""
    strings = _strings()
    assert len(strings) == 2 * sum(3 ** n for n in range(8)) + 10000 + 12
    exe = str(tmp_path / "token_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "token_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    valid = [0] * 8
    for c in sim_ref.DEFAULT_VALID:
        valid[c >> 5] |= 1 << (c & 31)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<8I", *valid) + struct.pack("<I", len(strings)))
        for cs, stored, s in strings:
            f.write(struct.pack("<BBI", cs, stored, len(s)))
            f.write(np.asarray(s, dtype=np.uint8 if cs == 1 else "<u4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip() == f"ok {len(strings)}", p.stdout
    data = open(dst, "rb").read()
    o = 0
    for i, (cs, stored, s) in enumerate(strings):
        (n,) = struct.unpack_from("<I", data, o)
        got = tuple(np.frombuffer(data, dtype=np.uint8 if cs == 1 else "<u4", count=n, offset=o + 4).tolist())
        o += 4 + n * cs
        assert got == token_ref.token_sort(s, wide=cs == 4, stored=bool(stored)), f"string {i} {s[:50]}"
    assert o == len(data)
