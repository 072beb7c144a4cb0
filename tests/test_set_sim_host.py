"""CPU-side checks of the later stages over an index set (no GPU compute): the new exports and their
bindings, the argument checks that answer before a set or the GPU is touched, the calls on unknown set
ids, and the host routines of stringsearchlib_amd/csrc/ngs_set.h (the member lookup and the record
rule) in a stand-alone program under ASan + UBSan against a numpy model."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from stringsearchlib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # a non-null "device pointer": the calls below fail before anything is read through it
HIP_INVALID_VALUE = 1
NGS_ERR_RERANK_LIMIT = 0x10003
UNKNOWN = 0x7FFF0000
NAN = float("nan")
NEW = ("ngsSetSimilarityDeviceM", "ngsSetRerankDeviceM", "ngsSetKeyQueryBytes", "ngsSetKeyQueriesDevice",
       "ngsSetSelfJoinDevice", "scoreBatchSetSimM", "scoreBatchSetSimMW", "scoreBatchSetSimMU8", "selfJoinSet",
       "dedupKeysSet")
BAD_METRICS = (3, 7, 0x103, 0x200, 0x80000000)


def test_header_declares_and_library_exports_the_symbols():
    syms = _native.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    L = _native.lib()
    for s in NEW:
        assert s in syms, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, f"{s} is not bound"
    import stringsearchlib_amd as ssl
    for m in ("score_batch_sim", "term", "self_join", "dedup", "similarity_device", "rerank_device", "key_query_bytes",
              "key_queries_device", "self_join_device"):
        assert callable(getattr(ssl.IndexSet, m)), m
    assert ssl.METRICS == {"levenshtein": 0, "osa": 1, "partial": 2}
    # the members' table travels in the kernel arguments: 16 x 56 bytes
    text = open(os.path.join(ROOT, "stringsearchlib_amd", "csrc", "ngs_sim.h")).read()
    assert re.search(r"static_assert\(sizeof\(SimMember\) == 56", text)


def test_device_forms_check_their_arguments_before_the_set():
    """Integers stand in for the device pointers, the set id is unknown: a bad argument answers -3, good
    ones -1, so every check comes before the set is looked at and before any HIP call."""
    L = _native.lib()

    def sim(off=P, n=4, stride=8, counts=P, keys=P, metric=0, out=P, terms=None):
        return L.ngsSetSimilarityDeviceM(UNKNOWN, P, off, n, stride, counts, keys, metric, out, terms, None)

    assert sim() == -1 and sim(terms=P) == -1 and sim(metric=0x102) == -1
    assert sim(off=None) == -3 and sim(counts=None) == -3 and sim(keys=None) == -3 and sim(out=None) == -3
    assert sim(n=0, keys=None, out=None) == -1 and sim(stride=0, keys=None, out=None) == -1  # no record: none needed
    for m in BAD_METRICS:
        assert sim(metric=m) == -3, m

    def rerank(off=P, n=4, stride=8, counts=P, keys=P, scores=P, out=P, metric=1, ms=0.5):
        return L.ngsSetRerankDeviceM(UNKNOWN, P, off, n, stride, counts, keys, scores, out, None, metric, ms, None)

    assert rerank() == -1 and rerank(stride=4096) == -1 and rerank(ms=-1.0) == -1
    assert rerank(off=None) == -3 and rerank(counts=None) == -3 and rerank(keys=None) == -3
    assert rerank(scores=None) == -3 and rerank(out=None) == -3
    assert rerank(stride=4097) == -3 and rerank(ms=NAN) == -3
    for m in BAD_METRICS:
        assert rerank(metric=m) == -3, m

    assert L.ngsSetKeyQueriesDevice(UNKNOWN, 0, 4, P, 64, None, None) == -3
    assert L.ngsSetKeyQueriesDevice(UNKNOWN, 0, 4, None, 64, P, None) == -3
    assert L.ngsSetKeyQueriesDevice(UNKNOWN, 0, 4, P, 64, P, None) == -1
    assert L.ngsSetKeyQueriesDevice(UNKNOWN, 0, 0, None, 0, P, None) == -1
    assert L.ngsSetKeyQueryBytes(UNKNOWN, 0, 4) == 0 and L.ngsSetKeyQueryBytes(UNKNOWN, 0, 0) == 0

    def join(n=4, counts=P, keys=P, scores=P):
        return L.ngsSetSelfJoinDevice(UNKNOWN, 0, n, 0.3, 10, 11, counts, keys, scores, None)

    assert join() == -1 and join(n=0, keys=None, scores=None) == -1
    assert join(counts=None) == -3 and join(keys=None) == -3 and join(scores=None) == -3


def test_host_forms_on_unknown_sets_and_bad_arguments():
    L = _native.lib()
    qs = (C.c_char_p * 2)(b"a", b"b")
    counts = (C.c_uint32 * 2)()
    keys, terms = (C.c_uint32 * 20)(), (C.c_uint32 * 20)()
    scores, sims = (C.c_float * 20)(), (C.c_float * 20)()
    forms = ((L.scoreBatchSetSimM, qs), (L.scoreBatchSetSimMU8, qs),
             (L.scoreBatchSetSimMW, C.cast(qs, C.POINTER(_native.W))))

    def fails(fn, q, metric=0, ms=0.0, t=terms, err=HIP_INVALID_VALUE):
        counts[0] = counts[1] = 9
        L.ngsLastError(1)
        assert fn(UNKNOWN, q, 2, 0.0, 10, metric, ms, 10, counts, keys, scores, sims, t) == 0
        assert L.ngsLastError(1) == err and list(counts) == [0, 0]

    for fn, q in forms:
        fails(fn, q)
        fails(fn, q, t=None)
        fails(fn, q, ms=NAN)
        for m in BAD_METRICS:
            fails(fn, q, metric=m)
        L.ngsLastError(1)
        assert fn(UNKNOWN, q, 2, 0.0, 10, 0, 0.0, 10, None, keys, scores, sims, terms) == 0  # no counts to zero
        assert L.ngsLastError(1) == HIP_INVALID_VALUE

    counts[0] = counts[1] = 9
    L.ngsLastError(1)
    assert L.selfJoinSet(UNKNOWN, 0, 2, 0.3, 10, 10, counts, keys, scores) == 0
    assert L.ngsLastError(1) == HIP_INVALID_VALUE and list(counts) == [0, 0]
    L.ngsLastError(1)
    assert L.selfJoinSet(UNKNOWN, 0, 2, 0.3, 10, 10, None, keys, scores) == 0 and L.ngsLastError(1) == HIP_INVALID_VALUE

    labels = (C.c_uint32 * 4)(7, 7, 7, 7)

    def dedup(limit=10, metric=0, ms=0.5, lab=labels):
        L.ngsLastError(1)
        assert L.dedupKeysSet(UNKNOWN, 0.3, limit, metric, ms, 0, lab) == 0
        return L.ngsLastError(1)

    assert dedup() == HIP_INVALID_VALUE and dedup(limit=4096) == HIP_INVALID_VALUE  # the set is unknown
    assert dedup(limit=0) == HIP_INVALID_VALUE and dedup(ms=NAN) == HIP_INVALID_VALUE
    assert dedup(lab=None) == HIP_INVALID_VALUE and dedup(limit=5000, lab=None) == HIP_INVALID_VALUE
    assert dedup(limit=4097) == NGS_ERR_RERANK_LIMIT
    for m in BAD_METRICS:
        assert dedup(metric=m) == HIP_INVALID_VALUE
    assert list(labels) == [7, 7, 7, 7]
    # set ids are not handles: an index handle of the same number is no set
    words = (C.c_char_p * 1)(b"seulement")
    h = L.indexN(words, 1, 1, None)  # an un-built handle, no GPU touched
    assert h
    try:
        assert L.ngsSetSimilarityDeviceM(h, P, P, 1, 1, P, P, 0, P, None, None) == -1
        assert L.ngsSetKeyQueryBytes(h, 0, 0) == 0 and L.ngsCharSize(h) == 1
    finally:
        L.dispose(h)


# ---- ngs_set.h's member lookup and record rule under sanitizers -----------------------------------------
NO_PART = 0xFFFFFFFF


def random_set(rng, sizes=None):
    """Members tiling [0, total): each with kt_off / kt_term (aliases: 0 to 4 terms a key, some ids at or past
    n_terms) or with the key_term map; some members empty."""
    sizes = sizes if sizes is not None else [rng.choice((0, 0, 1, 2, 5, 17, 64)) for _ in range(rng.randint(1, 16))]
    members, base = [], 0
    for nk in sizes:
        n_terms = rng.randint(1, 40)
        tid = lambda: rng.choice((rng.randrange(n_terms), rng.randrange(n_terms), n_terms, 0xFFFFFFFF))
        if rng.random() < 0.5:
            per = [rng.randint(0, 4) for _ in range(nk)]
            off = np.cumsum([0] + per).astype(np.uint32)
            m = {"form": 0, "kt_off": off, "kt_term": np.array([tid() for _ in range(int(off[-1]))], dtype=np.uint32)}
        else:
            m = {"form": 1, "key_term": np.array([tid() for _ in range(nk)], dtype=np.uint32)}
        m.update(n_keys=nk, n_terms=n_terms, base=base)
        members.append(m)
        base += nk
    return members, base


def probe_ids(rng, members, total):
    ids = {0, total - 1, total, total + 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000}
    for m in members:
        ids |= {m["base"] - 1, m["base"], m["base"] + m["n_keys"] - 1, m["base"] + m["n_keys"]}
    ids |= {rng.randrange(total + 3) for _ in range(20)}
    return sorted(g & 0xFFFFFFFF for g in ids if g >= 0)


def model(members, total, g):
    """(part, local key, the term ids the record compares): numpy's searchsorted over the bases for the part."""
    if g >= total:
        return NO_PART, 0, []
    bases = np.array([m["base"] for m in members], dtype=np.uint64)
    p = int(np.searchsorted(bases, g, side="right")) - 1
    m = members[p]
    assert m["base"] <= g < m["base"] + m["n_keys"]
    k = g - m["base"]
    ts = m["kt_term"][m["kt_off"][k]:m["kt_off"][k + 1]].tolist() if m["form"] == 0 else [int(m["key_term"][k])]
    return p, k, [t for t in ts if t < m["n_terms"]]


def record(members, ids):
    u32 = lambda *v: np.array(v, dtype="<u4").tobytes()
    body = [u32(len(members), len(ids))]
    for m in members:
        body.append(u32(m["form"], m["n_keys"], m["n_terms"], m["base"]))
        body += [m["kt_off"].astype("<u4").tobytes(), m["kt_term"].astype("<u4").tobytes()] if m["form"] == 0 else \
            [m["key_term"].astype("<u4").tobytes()]
    body.append(np.array(ids, dtype="<u4").tobytes())
    return b"".join(body)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_member_lookup_and_record_rule_under_sanitizers_match_the_model(tmp_path):
    """tests/sanitize/set_sim_driver.cpp (its own main, ngs_set.h alone, g++ -fsanitize=address,undefined) on
    sets of 1 to 16 members, empty ones included, at every base - 1, base, last key, total and 0xFFFFFFFF."""
    exe = str(tmp_path / "set_sim_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "set_sim_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    rng = random.Random(0x5E78)
    sets = [random_set(rng, s) for s in ([5], [0, 3], [3, 0], [2, 0, 0, 4, 0], [1] * 16, [0] * 3, [64, 1, 64])]
    sets += [random_set(rng) for _ in range(150)]
    records, want = [], []
    for members, total in sets:
        ids = probe_ids(rng, members, total)
        records.append(record(members, ids))
        for g in ids:
            p, k, ts = model(members, total, g)
            want += [p, k, len(ts)] + ts
    assert any(m["n_keys"] == 0 for ms, _ in sets for m in ms) and {len(ms) for ms, _ in sets} >= {1, 2, 3, 16}
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.strip() == f"ok {len(records)}", p.stdout
    got = np.frombuffer(open(dst, "rb").read(), dtype="<u4")
    exp = np.array(want, dtype=np.uint32)
    assert len(got) == len(exp)
    assert (got == exp).all(), np.flatnonzero(got != exp)[:5]
