"""CPU-side checks of the UTF-8 front end (no GPU compute): the eight new exports, their argument
checks, and the host codec (stringsearchlib_amd/csrc/ngs_utf8.h) under ASan + UBSan against
Python's decoder."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from stringsearchlib_amd import _native
from utf8_ref import all_two_byte, pool_four_byte, random_strings, ref_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8_EXPORTS = ["indexU8", "searchU8", "scoreU8", "searchBatchU8", "scoreBatchU8", "ngsKeyU8", "ngsUtf8Decode",
              "ngsSearchDeviceU8"]


def test_header_declares_and_library_exports_u8_symbols():
    syms = _native.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    L = _native.lib()
    for s in U8_EXPORTS:
        assert s in syms, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"


def test_u8_argument_checks_without_gpu_work():
    L = _native.lib()
    words = (C.c_char_p * 1)("seulement".encode())
    assert L.indexU8(words, 1, 1, None, 0) == 0 and L.indexU8(words, 1, 1, None, 4) == 0
    h = L.indexU8(words, 1, 1, None, 2)
    assert h
    try:
        assert L.ngsCharSize(h) == 4 and L.ngsGramSize(h) == 2
        assert L.getSizeW(h) == 0 and L.getLibSizeW(h) == 0
        res = C.POINTER(C.POINTER(C.c_char))()
        assert L.searchU8(h, "日本".encode(), C.byref(res), 0.0, 10) == 0 and not res
        sc = C.POINTER(C.c_float)()
        assert L.scoreU8(h, b"x", C.byref(res), C.byref(sc), 0.0, 10) == 0 and not res and not sc
        counts = (C.c_uint32 * 2)(7, 7)
        qs = (C.c_char_p * 2)(b"a", b"b")
        assert L.scoreBatchU8(h, qs, 2, 0.0, 10, counts, C.byref(res), C.byref(sc)) == 0 and not res
        assert list(counts) == [0, 0]
        assert not L.ngsKeyU8(h, 0)
        assert L.ngsSearchDeviceU8(h, None, None, 0, 0.0, 10, 10, None, None, None, None) == -2
    finally:
        L.dispose(h)
    # a narrow un-built handle, and an unknown one
    n = L.indexN(words, 1, 1, None)
    assert n
    try:
        res = C.POINTER(C.POINTER(C.c_char))()
        assert L.searchU8(n, b"seulement", C.byref(res), 0.0, 10) == 0 and not res
        assert not L.ngsKeyU8(n, 0)
    finally:
        L.dispose(n)
    assert L.searchU8(n + 1000, b"x", C.byref(res), 0.0, 10) == 0
    assert L.ngsSearchDeviceU8(n + 1000, None, None, 0, 0.0, 10, 10, None, None, None, None) == -1
    # ngsUtf8Decode checks its arguments before it touches a device
    assert L.ngsUtf8Decode(None, None, 0, None, 0, None, None) == -3
    assert L.ngsUtf8Decode(None, None, 4, None, 64, None, None) == -3


def _codec_inputs():
    return all_two_byte() + pool_four_byte() + random_strings(20000, seed=0x5EED)


def _run_driver(exe, strings, tmp_path):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(strings)))
        f.write(b"".join(bytes((len(s),)) + s for s in strings))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip().startswith(f"ok {len(strings)} "), p.stdout
    return np.fromfile(dst, dtype="<u4")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_host_codec_under_sanitizers_matches_python(tmp_path):
    """tests/sanitize/utf8_driver.cpp (its own main, g++ alone, -fsanitize=address,undefined) decodes
    all 65,536 two-byte strings, all 4-byte strings over the boundary pool and 20k seeded random
    strings of 0..40 bytes; its units equal Python's, and the driver itself checks the inverse
    (encode(decode(s)) == s), utf8_encoded_len and the per-byte rule on every string."""
    exe = str(tmp_path / "utf8_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "utf8_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    strings = _codec_inputs()
    assert len(strings) == 65536 + 25 ** 4 + 20000
    got = _run_driver(exe, strings, tmp_path)
    want = []
    for s in strings:
        u = ref_units(s)
        want.append(len(u))
        want.extend(u)
    want = np.asarray(want, dtype="<u4")
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first difference at word {bad[0]}: {got[bad[0]]:#x} vs {want[bad[0]]:#x}"
