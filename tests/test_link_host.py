"""CPU-side checks of linking two indexes (no GPU compute): the new exports and their bindings, the
argument checks that answer before anything is read, the model's rounds against its sequential greedy
(tests/match_ref.py), and the host routines of stringsearchlib_amd/csrc/ngs_match.h in a stand-alone
program under ASan + UBSan against the model."""
import ctypes as C
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import match_cases
import match_ref
from stringsearchlib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # a non-null "device pointer": the calls below fail before anything is read through it
NGS_ERR_RERANK_LIMIT = 0x10003
HIP_INVALID_VALUE = 1
CASES = match_cases.cases()


def case_rows(case):
    name, n_a, n_b, first, n, stride, counts, keys, values = case
    return match_ref.block_rows(counts, keys, values.view(np.uint32), n, stride, first, n_a, n_b)


def test_header_declares_and_library_exports_link_symbols():
    syms = _native.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    L = _native.lib()
    for s in ("ngsMatchDevice", "linkKeys"):
        assert s in syms, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"
    header = open(_native.HEADER).read()
    for name, value in (("NGS_NO_MATCH", "0xFFFFFFFFu"), ("NGS_MATCH_INIT", "1u"), ("NGS_MATCH_BEGIN", "2u"),
                        ("NGS_MATCH_BID", "4u"), ("NGS_MATCH_ACCEPT", "8u"), ("NGS_LINK_BEST", "0u"),
                        ("NGS_LINK_ONE_TO_ONE", "1u")):
        assert re.search(rf"#define\s+{name}\s+{value}\b", header), name
    assert "Linking two indexes" in header
    import stringsearchlib_amd as ssl
    assert ssl.NO_MATCH == 0xFFFFFFFF and "NO_MATCH" in ssl.__all__
    for m in ("link", "match_device"):
        for cls in (ssl.StringIndex, ssl.WideStringIndex, ssl.Utf8StringIndex):
            assert callable(getattr(cls, m)), (cls, m)


def test_match_device_argument_checks_without_gpu_work():
    """Integers stand in for the device pointers: every call answers -3 before any HIP call."""
    L = _native.lib()
    ok = dict(c=P, k=P, v=P, n=4, stride=8, first=0, ma=P, na=16, mb=P, nb=16, bids=P, matched=P, flags=15)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ngsMatchDevice(a["c"], a["k"], a["v"], a["n"], a["stride"], a["first"], a["ma"], a["na"], a["mb"],
                                a["nb"], a["bids"], a["matched"], a["flags"], None)

    assert call(flags=16) == -3 and call(flags=0x8000000F) == -3   # an unknown flag
    assert call(matched=None) == -3 and call(matched=None, n=0, flags=0) == -3
    assert call(ma=None) == -3                                       # sources and no array
    assert call(mb=None) == -3 and call(bids=None) == -3             # targets and no array
    for flags in (4, 8, 12, 15):                                     # rows to read
        assert call(c=None, flags=flags) == -3
        assert call(k=None, flags=flags) == -3
        assert call(v=None, flags=flags) == -3
    assert call(flags=1, ma=None, na=0, mb=None, nb=16) == -3


def test_link_keys_failure_table_without_gpu_work():
    L = _native.lib()
    words = (C.c_char_p * 1)(b"seulement")
    h = L.indexN(words, 1, 1, None)  # one word: an un-built handle, no GPU touched
    w0 = (C.c_uint32 * 10)(*map(ord, "seulement"), 0)
    wide = (_native.W * 1)(C.cast(w0, _native.W))
    hw = L.indexW(wide, 1, 1, None, 2)
    assert h and hw
    match = (C.c_uint32 * 4)(9, 9, 9, 9)
    scores = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    sims = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)

    def fails(err, h_from=h, h_to=h, limit=10, metric=0, min_sim=-1.0, mode=1, m=match):
        L.ngsLastError(1)
        assert L.linkKeys(h_from, h_to, 0.5, limit, metric, min_sim, mode, 0, m, scores, sims) == 0
        assert L.ngsLastError(1) == err
        assert list(match) == [9] * 4 and list(scores) == [7.0] * 4 and list(sims) == [7.0] * 4

    try:
        # the arguments, before the handles are looked up (unknown handles here)
        bad = h + hw + 1000
        fails(HIP_INVALID_VALUE, bad, bad, m=None)
        fails(HIP_INVALID_VALUE, bad, bad, limit=0)
        fails(NGS_ERR_RERANK_LIMIT, bad, bad, limit=4097)
        fails(HIP_INVALID_VALUE, bad, bad, limit=4097, m=None)
        fails(HIP_INVALID_VALUE, bad, bad, min_sim=float("nan"))
        for metric in (3, 0x103, 0x200, 0xFFFFFFFF):
            fails(HIP_INVALID_VALUE, bad, bad, metric=metric)
        for mode in (2, 0xFFFFFFFF):
            fails(HIP_INVALID_VALUE, bad, bad, mode=mode)
        # the handles: unknown, un-built, of two widths
        fails(HIP_INVALID_VALUE, bad, bad)
        fails(HIP_INVALID_VALUE, bad, h)
        fails(HIP_INVALID_VALUE, h, bad)
        for mode in (0, 1):
            fails(HIP_INVALID_VALUE, h, h, mode=mode)
            fails(HIP_INVALID_VALUE, h, hw, mode=mode)
            fails(HIP_INVALID_VALUE, hw, h, mode=mode)
            fails(HIP_INVALID_VALUE, hw, hw, mode=mode, metric=0x101, min_sim=0.5)
    finally:
        L.dispose(h)
        L.disposeW(hw)


# ---- the model against itself ----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_rounds_equal_model_greedy_on_the_cases(case):
    name, n_a, n_b = case[:3]
    rows = case_rows(case)
    want = match_ref.greedy(n_a, n_b, rows)
    pairs = sum(1 for b in want[0] if b != match_ref.NO_MATCH)
    assert pairs > 0 and all(want[1][b] == a for a, b in enumerate(want[0]) if b != match_ref.NO_MATCH)
    for rng in (None, random.Random(1), random.Random(2)):
        ma, mb, count = match_ref.rounds(n_a, n_b, rows, rng)
        assert (ma, mb) == want, name
        if name == "chain":
            assert count == 71 and pairs == 70
        if name == "contention":  # (a row that sees row 0's match takes its second choice in the same round)
            assert count in (2, 3) and pairs == 1000 and ma[0] == 0 and ma[1:] == list(range(2, 1001))
    if name.startswith("random"):
        # the case holds what it is meant to: ids past both arrays, counts above the stride, a b twice in a row,
        # and ties that the order of a decides
        n, stride, counts, keys = case[4], case[5], case[6], case[7]
        assert case[3] + n > n_a and (counts > stride).any()
        live = [keys[i * stride:i * stride + min(int(counts[i]), stride)] for i in range(n)]
        assert any((r >= n_b).any() for r in live)
        assert stride == 1 or any(len(set(r.tolist())) < len(r) for r in live)
        assert match_ref.best(n_a, rows) != want[0]


def test_model_rounds_equal_model_greedy_on_random_small_blocks():
    """3,000 small bipartite blocks with tied values, ACCEPT in shuffled row order against the mid-round state."""
    rng = random.Random(0x9E6)
    for t in range(3000):
        n_a, n_b = rng.randrange(1, 9), rng.randrange(1, 9)
        rows = {a: [(match_ref.order_bits(np.float32(rng.choice(match_cases.VALUES)).view(np.uint32)), rng.randrange(n_b))
                    for _ in range(rng.randrange(0, 5))] for a in range(n_a) if rng.random() < 0.9}
        want = match_ref.greedy(n_a, n_b, rows)
        ma, mb, count = match_ref.rounds(n_a, n_b, rows, rng)
        assert (ma, mb) == want, (t, rows)
        assert count <= sum(1 for b in ma if b != match_ref.NO_MATCH) + 1  # every round but the last adds a pair


def test_order_bits_is_the_floats_order():
    vals = np.array([-np.inf, -1.0, -1e-30, -0.0, 0.0, 1e-30, 0.25, 1.0, np.inf], dtype=np.float32)
    img = [match_ref.order_bits(b) for b in vals.view(np.uint32)]
    assert img == sorted(img) and len(set(img)) == len(img)


# ---- ngs_match.h under sanitizers --------------------------------------------------------------------
def _build_driver(tmp_path):
    exe = str(tmp_path / "match_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "match_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_host_match_routines_under_sanitizers_match_model(tmp_path):
    """tests/sanitize/match_driver.cpp (its own main, ngs_match.h alone, g++ -fsanitize=address,undefined):
    match_greedy, and match_round over one block and over several, on every case; the output must be
    the model's, the rounds included."""
    exe = _build_driver(tmp_path)
    u32 = lambda *v: struct.pack(f"<{len(v)}I", *v)
    records, want = [], []
    for case in CASES:
        name, n_a, n_b, first, n, stride, counts, keys, values = case
        ma, mb, count = match_ref.rounds(n_a, n_b, case_rows(case))
        assert (ma, mb) == match_ref.greedy(n_a, n_b, case_rows(case))
        pairs = sum(1 for b in ma if b != match_ref.NO_MATCH)
        body = counts.tobytes() + keys.tobytes() + values.tobytes()
        records.append(u32(1, n_a, n_b, n, stride, first) + body)
        want.append(ma + mb + [pairs])
        for cuts in ([0, n], match_cases.cuts_of(n, n + stride)):
            records.append(u32(2, n_a, n_b, n, stride, first, len(cuts) - 1, *cuts) + body)
            want.append(ma + mb + [pairs, count])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip() == f"ok {len(records)}", p.stdout
    got = np.frombuffer(open(dst, "rb").read(), dtype="<u4")
    flat = np.array([x for w in want for x in w], dtype="<u4")
    assert len(got) == len(flat)
    assert (got == flat).all(), np.flatnonzero(got != flat)[:5]
