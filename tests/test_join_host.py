"""CPU-side checks of the self-join (no GPU compute): the new exports and their bindings, the
argument checks that answer before anything is read, and the host routines of
stringsearchlib_amd/csrc/ngs_join.h (offset formula, drop-self on a row, union and find) in a
stand-alone program under ASan + UBSan against tests/join_ref.py."""
import ctypes as C
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import join_cases
import join_ref
from stringsearchlib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN_EXPORTS = ["ngsKeyQueryBytes", "ngsKeyQueriesDevice", "ngsDropSelfDevice", "ngsSelfJoinDevice",
                "ngsClusterDevice", "selfJoin", "dedupKeys"]
P = 0x1000  # a non-null "device pointer": the calls below fail before anything is read through it
NGS_ERR_RERANK_LIMIT = 0x10003
HIP_INVALID_VALUE = 1


def test_header_declares_and_library_exports_join_symbols():
    syms = _native.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    L = _native.lib()
    for s in JOIN_EXPORTS:
        assert s in syms, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"
    header = open(_native.HEADER).read()
    assert re.search(r"#define\s+NGS_CLUSTER_INIT\s+1u\b", header)
    assert re.search(r"#define\s+NGS_CLUSTER_FINISH\s+2u\b", header)
    import stringsearchlib_amd as ssl
    for m in ("self_join", "dedup", "key_query_bytes", "key_queries_device", "drop_self_device", "self_join_device",
              "cluster_device"):
        for cls in (ssl.StringIndex, ssl.WideStringIndex, ssl.Utf8StringIndex):
            assert callable(getattr(cls, m)), (cls, m)


def test_join_argument_checks_without_gpu_work():
    L = _native.lib()
    words = (C.c_char_p * 1)(b"seulement")
    h = L.indexN(words, 1, 1, None)  # one word: an un-built handle, no GPU touched
    assert h
    labels = (C.c_uint32 * 4)(9, 9, 9, 9)
    try:
        # bad arguments answer before the handle is looked at
        assert L.ngsKeyQueriesDevice(h, 0, 1, P, 64, None, None) == -3    # null offsets
        assert L.ngsKeyQueriesDevice(h, 0, 1, None, 64, P, None) == -3    # a capacity and no buffer
        assert L.ngsSelfJoinDevice(h, 0, 1, 0.5, 10, 11, None, P, P, None) == -3  # null counts
        assert L.ngsSelfJoinDevice(h, 0, 1, 0.5, 10, 11, P, None, P, None) == -3  # null keys
        assert L.ngsSelfJoinDevice(h, 0, 1, 0.5, 10, 11, P, P, None, None) == -3  # null scores
        # then the handle: un-built
        assert L.ngsKeyQueryBytes(h, 0, 1) == 0
        assert L.ngsKeyQueriesDevice(h, 0, 1, P, 64, P, None) == -2
        assert L.ngsKeyQueriesDevice(h, 0, 0, None, 0, P, None) == -2
        assert L.ngsSelfJoinDevice(h, 0, 1, 0.5, 10, 11, P, P, P, None) == -2
        counts = (C.c_uint32 * 2)(7, 7)
        L.ngsLastError(1)
        assert L.selfJoin(h, 0, 2, 0.5, 10, 10, counts, counts, C.cast(counts, C.POINTER(C.c_float))) == 0
        assert list(counts) == [0, 0] and L.ngsLastError(1) == HIP_INVALID_VALUE
        assert L.dedupKeys(h, 0.5, 10, -1.0, 0, labels) == 0
        assert L.ngsLastError(1) == HIP_INVALID_VALUE and list(labels) == [9, 9, 9, 9]
    finally:
        L.dispose(h)
    # ... or unknown
    assert L.ngsKeyQueryBytes(h + 1000, 0, 1) == 0
    assert L.ngsKeyQueriesDevice(h + 1000, 0, 1, P, 64, P, None) == -1
    assert L.ngsSelfJoinDevice(h + 1000, 0, 1, 0.5, 10, 11, P, P, P, None) == -1
    counts = (C.c_uint32 * 2)(7, 7)
    assert L.selfJoin(h + 1000, 0, 2, 0.5, 10, 10, counts, counts, C.cast(counts, C.POINTER(C.c_float))) == 0
    assert list(counts) == [0, 0] and L.ngsLastError(1) == HIP_INVALID_VALUE
    # dedupKeys: the limit and the similarity bound are checked like the handle, before any work
    for lim, sim, err in ((0, -1.0, HIP_INVALID_VALUE), (4097, -1.0, NGS_ERR_RERANK_LIMIT),
                          (10, float("nan"), HIP_INVALID_VALUE)):
        assert L.dedupKeys(h + 1000, 0.5, lim, sim, 0, labels) == 0
        assert L.ngsLastError(1) == err
    assert L.dedupKeys(h + 1000, 0.5, 10, 0.5, 0, None) == 0 and L.ngsLastError(1) == HIP_INVALID_VALUE
    # the two stages without a handle
    assert L.ngsDropSelfDevice(None, P, P, 4, 8, 0, 0, None) == -3   # null counts
    assert L.ngsDropSelfDevice(P, None, P, 4, 8, 0, 0, None) == -3   # null keys with cells to read
    assert L.ngsDropSelfDevice(P, P, None, 4, 8, 0, 0, None) == -3   # null scores
    assert L.ngsClusterDevice(P, P, 4, 8, 0, P, 16, 4, None) == -3   # an unknown flag
    assert L.ngsClusterDevice(P, P, 4, 8, 0, None, 16, 3, None) == -3  # labels to write and no array
    assert L.ngsClusterDevice(None, P, 4, 8, 0, P, 16, 3, None) == -3  # null counts with rows to read
    assert L.ngsClusterDevice(P, None, 4, 8, 0, P, 16, 3, None) == -3  # null keys
    assert L.ngsClusterDevice(None, None, 0, 8, 0, None, 0, 3, None) == 0  # no rows, no labels: nothing to queue


def _build_driver(tmp_path):
    exe = str(tmp_path / "join_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "join_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def _run_driver(exe, tmp_path, records):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip() == f"ok {len(records)}", p.stdout
    return open(dst, "rb").read()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_host_join_routines_under_sanitizers_match_reference(tmp_path):
    """tests/sanitize/join_driver.cpp (its own main, ngs_join.h alone, g++ -fsanitize=address,undefined)
    against join_ref: the offsets, every drop-self row of join_cases, every cluster case in one block
    and split over three."""
    exe = _build_driver(tmp_path)
    u32 = lambda *v: struct.pack(f"<{len(v)}I", *v)
    records, checks = [], []

    # 1. offsets: keys of the lengths the gather test uses, narrow and wide, whole and sub-ranges
    rng = random.Random(11)
    lens = [1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 300, 1, 3, 5] + [rng.randrange(1, 40) for _ in range(50)]
    key_off = [0]
    for n in lens:
        key_off.append(key_off[-1] + n + 1)  # one NUL per key
    for cs in (1, 4):
        for first, n in ((0, len(lens)), (len(lens) - 1, 1), (5, 0), (7, 13), (len(lens), 0)):
            records.append(u32(1, len(lens), first, n, cs) + struct.pack(f"<{len(key_off)}Q", *key_off))
            want = join_ref.query_offsets(lens[first:first + n], cs)
            assert want == join_ref.offsets_from_key_off(key_off, first, n, cs)
            checks.append(("Q", want))

    # 2. drop-self
    for stride in join_cases.DROP_STRIDES:
        counts, keys, scores = join_cases.drop_block(stride)
        for limit in join_cases.drop_limits(stride):
            for i, c in enumerate(counts):
                rk, rs = keys[i * stride:(i + 1) * stride], scores[i * stride:(i + 1) * stride]
                records.append(u32(2, int(c), stride, join_cases.DROP_FIRST + i, limit) + rk.tobytes() + rs.tobytes())
                checks.append(("drop", stride, join_ref.drop_self(rk, rs.view(np.uint32), int(c), stride,
                                                                  join_cases.DROP_FIRST + i, limit)))

    # 3. clusters: one block, then three
    for name, n_labels, first, n, stride, counts, keys in join_cases.cluster_cases():
        want = join_ref.labels(n_labels, join_ref.block_edges(counts, keys, n, stride, first))
        records.append(u32(3, 3, n_labels, n, stride, first) + counts.tobytes() + keys.tobytes())
        checks.append(("I", want))
        cuts = [0, n // 3, n // 3, n]  # (an empty block in the middle)
        for j in range(3):
            a, b = cuts[j], cuts[j + 1]
            flags = (1 if j == 0 else 0) | (2 if j == 2 else 0)
            records.append(u32(3, flags, n_labels, b - a, stride, first + a) + counts[a:b].tobytes() +
                           keys[a * stride:b * stride].tobytes())
            checks.append(("I", want) if j == 2 else None)

    got = _run_driver(exe, tmp_path, records)
    at = 0
    for c in checks:
        if c is None:
            continue
        if c[0] in "QI":
            w = np.array(c[1], dtype="<u8" if c[0] == "Q" else "<u4")
            g = np.frombuffer(got, dtype=w.dtype, count=len(w), offset=at)
            assert (g == w).all(), (c[0], np.flatnonzero(g != w)[:5])
            at += w.nbytes
        else:
            _, stride, (kept, wk, ws) = c
            g = np.frombuffer(got, dtype="<u4", count=1 + 2 * stride, offset=at)
            assert g[0] == kept
            assert g[1:1 + kept].tolist() == wk and g[1 + stride:1 + stride + kept].tolist() == ws
            at += 4 * (1 + 2 * stride)
    assert at == len(got)
