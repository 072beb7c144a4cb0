"""CPU-side checks of the edit-distance similarity stage (no GPU compute): the new exports, their
argument checks, and the host routines of stringsearchlib_amd/csrc/ngs_sim.h (normalisation, the
one-word and the multi-word global Myers recurrence, the fp32 sim) under ASan + UBSan against
tests/sim_ref.py."""
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

import sim_ref
from stringsearchlib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_EXPORTS = ["ngsSimilarityDevice", "ngsRerankDevice", "scoreBatchSim", "scoreBatchSimW", "scoreBatchSimU8"]
P = 0x1000  # a non-null "device pointer": the calls below fail before anything is read through it


def test_header_declares_and_library_exports_sim_symbols():
    syms = _native.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    L = _native.lib()
    for s in SIM_EXPORTS:
        assert s in syms, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"
    header = open(_native.HEADER).read()
    assert re.search(r"#define\s+NGS_ERR_RERANK_LIMIT\s+0x10003\b", header)


def test_sim_argument_checks_without_gpu_work():
    L = _native.lib()
    words = (C.c_char_p * 1)(b"seulement")
    h = L.indexN(words, 1, 1, None)  # one word: an un-built handle, no GPU touched
    assert h
    try:
        assert L.ngsSimilarityDevice(h, P, P, 4, 8, P, P, P, None) == -2
        assert L.ngsRerankDevice(h, P, P, 4, 8, P, P, P, P, 0.5, None) == -2
        # bad arguments answer before the handle is looked at
        assert L.ngsSimilarityDevice(h, P, P, 4, 8, None, P, P, None) == -3  # null dCounts
        assert L.ngsRerankDevice(h, P, P, 4, 8, None, P, P, P, 0.5, None) == -3
        assert L.ngsSimilarityDevice(h, P, None, 4, 8, P, P, P, None) == -3  # null offsets
        assert L.ngsSimilarityDevice(h, P, P, 4, 8, P, None, P, None) == -3  # null keys with records to read
        assert L.ngsSimilarityDevice(h, P, P, 4, 8, P, P, None, None) == -3  # null dSim
        assert L.ngsRerankDevice(h, P, P, 4, 8, P, P, None, P, 0.5, None) == -3  # null dScores
        assert L.ngsRerankDevice(h, P, P, 4, 4097, P, P, P, P, 0.5, None) == -3  # stride above kRerankMaxStride
        assert L.ngsRerankDevice(h, P, P, 4, 4096, P, P, P, P, 0.5, None) == -2
        assert L.ngsRerankDevice(h, P, P, 4, 8, P, P, P, P, float("nan"), None) == -3
        # scoreBatchSim on an un-built handle: 0, counts zeroed, outputs untouched
        res = C.POINTER(C.POINTER(C.c_char))()
        sc, sv = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        counts = (C.c_uint32 * 2)(7, 7)
        qs = (C.c_char_p * 2)(b"a", b"b")
        assert L.scoreBatchSim(h, qs, 2, 0.0, 10, 0.5, counts, C.byref(res), C.byref(sc), C.byref(sv)) == 0
        assert list(counts) == [0, 0] and not res and not sc and not sv
        counts = (C.c_uint32 * 2)(7, 7)
        assert L.scoreBatchSimU8(h, qs, 2, 0.0, 10, 0.5, counts, C.byref(res), C.byref(sc), C.byref(sv)) == 0
        assert list(counts) == [0, 0] and not res and not sv
    finally:
        L.dispose(h)
    assert L.ngsSimilarityDevice(h + 1000, P, P, 4, 8, P, P, P, None) == -1
    assert L.ngsRerankDevice(h + 1000, P, P, 4, 8, P, P, P, P, 0.5, None) == -1
    counts = (C.c_uint32 * 2)(7, 7)
    assert L.scoreBatchSim(h + 1000, qs, 2, 0.0, 10, 0.5, counts, C.byref(res), C.byref(sc), C.byref(sv)) == 0
    assert list(counts) == [0, 0]


def test_reference_batch_dp_equals_the_plain_two_row_dp():
    rng = random.Random(7)
    qs = [tuple(rng.choice(b"ACGT") for _ in range(rng.randint(0, 30))) for _ in range(400)]
    ts = [tuple(rng.choice(b"ACGT") for _ in range(rng.randint(0, 30))) for _ in range(400)]
    got = sim_ref.lev_batch(qs, ts)
    assert [int(x) for x in got] == [sim_ref.lev(q, t) for q, t in zip(qs, ts)]
    assert sim_ref.lev(b"kitten", b"sitting") == 3 and sim_ref.lev(b"", b"abc") == 3
    assert sim_ref.normalise(b"  a#b\t") == tuple(b"A B") and sim_ref.normalise(b"#\x80 ") == ()


def _pairs():
    """(raw query, term) pairs: all over {A, B} with lengths 0..6 on both sides, 20,000 seeded random
    ones of lengths 1..80 over four letters, and the word-boundary lengths."""
    short = [bytes(t) for n in range(7) for t in itertools.product(b"AB", repeat=n)]
    pairs = [(q, t) for q in short for t in short]
    rng = random.Random(0x51A1)
    rs = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    pairs += [(rs(rng.randint(1, 80)), rs(rng.randint(1, 80))) for _ in range(20000)]
    for m in (63, 64, 65, 127, 128, 129):
        for ln in (1, 63, 64, 65, 200):
            q = rs(m)
            pairs += [(q, rs(ln)), (q, q[:ln] if ln <= m else q + rs(ln - m)), (q, (q[:-1] + b"%")[:max(ln, 1)])]
    # raw forms the normalisation changes: blanks and invalid bytes to trim, lower case, nothing left
    pairs += [(b"  ab#c\t\n", b"AB C"), (b"#\x80ab\xff ", b"AB"), (b" \t ", b"ABC"), (b"*", b"ABC"), (b"**", b"A"),
              (b"a" * 64 + b" ", b"A" * 64), (b" " + b"a" * 65, b"A" * 64)]
    return pairs


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_host_similarity_under_sanitizers_matches_reference(tmp_path):
    """tests/sanitize/sim_driver.cpp (its own main, ngs_sim.h alone, g++ -fsanitize=address,undefined)
    against sim_ref: the distance and the fp32 bits of sim from the one-word and the multi-word routine."""
    exe = str(tmp_path / "sim_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "sim_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    pairs = _pairs()
    assert len(pairs) == 127 * 127 + 20000 + 90 + 7
    valid = [0] * 8
    for c in sim_ref.DEFAULT_VALID:
        valid[c >> 5] |= 1 << (c & 31)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I8I", len(pairs), *valid))
        f.write(b"".join(struct.pack("<H", len(q)) + q + struct.pack("<H", len(t)) + t for q, t in pairs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip() == f"ok {len(pairs)}", p.stdout
    got = np.fromfile(dst, dtype="<u4").reshape(len(pairs), 4)
    # the reference: normalise, two-row DP, float32 arithmetic
    qn = [None if sim_ref.is_wildcard(q) else sim_ref.normalise(q) for q, _ in pairs]
    live = [i for i, q in enumerate(qn) if q is not None]
    d = sim_ref.lev_batch([qn[i] for i in live], [tuple(pairs[i][1]) for i in live])
    want = np.zeros((len(pairs), 4), dtype=np.uint32)
    want[:, 0] = want[:, 2] = 0xFFFFFFFF
    want[:, 1] = want[:, 3] = np.float32(1.0).view(np.uint32)
    for i, di in zip(live, d):
        m, ln = len(qn[i]), len(pairs[i][1])
        b = np.float32(sim_ref.sim_value(int(di), m, ln)).view(np.uint32)
        want[i] = (di, b, di, b) if m <= 64 else (0xFFFFFFFF, 0, di, b)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"pair {bad[0]} {pairs[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"
