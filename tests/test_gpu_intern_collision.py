"""The device build's deferral on a 64-bit hash collision (ngs_intern.hip: k_check raises
kInternCollision, the build runs on over the merged runs, reads the flag and returns to the host
build), reached with the planted strings of tests/golden/collisions/intern_collisions.json.

tests/hash_cases.py makes seven small wide corpora from them: colliding terms (short, and long
ones that share 8 characters), colliding keys, both, lengths 4 and 3 in one run, runs A, B, A, and
a control that differs from the fourth in one character per pair. tests/test_hash_cases.py proves
on the CPU where each collides. tests/test_gpu_build_ref.py compares every array of the first six
with the independent model. Here each corpus runs as a wide index at gram sizes 2 and 3 and as a
UTF-8 index, and must

* print the phases of a deferred build under NGS_BUILD_TIMING (the blob went to HBM, the GPU phases
  never finished, the host parsed and interned), the control those of a device build;
* have the model's getSize, getLibSize and key count, the model's keys and terms one by one (both
  strings of a colliding pair apart), and the digest of an NGS_HOST_INTERN=1 build;
* answer like the generic oracle.

The later stages run on a deferred index (similarity re-rank against tests/sim_ref.py, dedup
against tests/join_ref.py), and thirty deferred builds of an 8 MB library leave no device memory
behind (the early return frees the build's arena).
"""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import build_ref
import hash_cases as hc
import join_ref
import sim_ref
import stringsearchlib_amd as ssl
from oracle_py import OracleIndexG
from stringsearchlib_amd import _native

pytestmark = pytest.mark.gpu

CORPORA = hc.collision_corpora()
SHAPES = [("w", 2), ("w", 3), ("u8", 2)]
SETTINGS = [(0.0, 7), (0.3, 100)]


def _text(words):
    return [None if w is None else hc.text(w) for w in words]


def _build(words, rs, wts, shape, env=None):
    """The index of `shape`; `env` is set for this build only."""
    kind, g = shape
    cls = ssl.WideStringIndex if kind == "w" else ssl.Utf8StringIndex
    if env:
        os.environ[env] = "1"
    try:
        return cls(_text(words), rs, wts, gram_size=g)
    finally:
        if env:
            os.environ.pop(env, None)


def _digest(idx):
    out = (C.c_uint64 * 20)()
    assert _native.lib().ngsIndexDigest(idx.handle, out, 20) == 20
    return list(out)


def _phases(err):
    return [line.split("]", 1)[1].rsplit(None, 2)[0].strip() for line in err.splitlines() if line.startswith("[ngs build]")]


def _assert_deferred(err, deferred, what):
    ph = _phases(err)
    if deferred:
        assert "intern: blob to HBM" in ph and "parse+intern" in ph, f"{what}: no deferral to the host build: {ph}"
        assert "intern: GPU phases" not in ph and "intern + CSR (GPU)" not in ph, f"{what}: the device build finished: {ph}"
    else:
        assert "intern + CSR (GPU)" in ph and "intern: GPU phases" in ph and "parse+intern" not in ph, f"{what}: {ph}"


def _collision_runs(strings):
    by = {}
    for s in strings:
        by.setdefault(hc.d_hash(s), set()).add(tuple(s))
    return [v for v in by.values() if len(v) > 1]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}{s[1]}")
@pytest.mark.parametrize("name", hc.DEFERRING + [hc.CONTROL])
def test_collision_defers_to_the_host_build(name, shape, capfd):
    words, rs, wts = CORPORA[name]
    g = shape[1]
    what = f"{name} {shape[0]}{g}"
    m = build_ref.build(words, rs, wts, g=g, wide=True)
    capfd.readouterr()
    idx = _build(words, rs, wts, shape, "NGS_BUILD_TIMING")
    try:
        _assert_deferred(capfd.readouterr().err, name != hc.CONTROL, what)
        assert (idx.size(), idx.lib_size(), idx.num_keys()) == (len(m.terms), m.n_grams, len(m.keys)), what
        keys = [idx.key(k) for k in range(idx.num_keys())]
        assert keys == [hc.text(k) for k in m.keys], what
        terms = [idx.term(t) for t in range(idx.size())]
        assert terms == [hc.text(t) for t in m.terms], what
        for run in _collision_runs(m.keys):
            assert all(keys.count(hc.text(s)) == 1 for s in run), f"{what}: colliding keys are not one key each"
        for run in _collision_runs(m.terms):
            assert all(terms.count(hc.text(s)) == 1 for s in run), f"{what}: colliding terms are not one term each"
        host = _build(words, rs, wts, shape, "NGS_HOST_INTERN")
        try:
            assert _digest(idx) == _digest(host), what
        finally:
            host.dispose()
        oi = OracleIndexG(words, rs, wts, g=g, wide=True)
        assert (oi.size(), oi.lib_size(), oi.n_keys()) == (len(m.terms), m.n_grams, len(m.keys)), what
        queries = sorted({hc.text(w) for w in words if w is not None})
        queries += [q.lower() for q in queries[:4]] + [q[:-1] for q in queries[:6]] + ["*", ""]
        for thr, lim in SETTINGS:
            got = idx.score_batch(queries, thr, lim)
            for q, a in zip(queries, got):
                ref = oi.score(q, thr, lim)
                assert a == ref, f"{what}: query {q!r} at ({thr}, {lim}): {a[:4]} vs oracle {ref[:4]}"
    finally:
        idx.dispose()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}{s[1]}")
def test_query_for_one_of_a_long_pair_returns_both_keys(shape):
    """collide_terms_long: the two terms of a pair share their last 8 characters, so a query equal to
    one returns both keys. The key that is its own term (no lower-case letter: the promotion compares
    the key as it is with the upper-cased query, nGramSearch.hpp:330-334) is promoted to 100; the
    other key's query finds its term whole (score = its weight) and is not promoted."""
    words, rs, wts = CORPORA["collide_terms_long"]
    fx = hc.load_collisions()
    idx = _build(words, rs, wts, shape)
    try:
        for a, b in fx["same_length_before_tail"][:4]:
            lower, upper = hc.text(a) + hc.SUFFIX.lower(), hc.text(b) + hc.SUFFIX
            got = idx.score(upper, 0.3, 100)
            assert got[0] == (upper, 100.0), (shape, upper, got[:3])
            assert lower in [k for k, _ in got[1:]] and all(s < 100.0 for _, s in got[1:]), (shape, upper, got)
            got = dict(idx.score(lower, 0.3, 100))
            assert got[lower] == wts[words.index(hc._a(lower))] and upper in got, (shape, lower, got)
            assert max(got.values()) < 100.0
    finally:
        idx.dispose()


@pytest.mark.parametrize("g", [2, 3])
def test_later_stages_on_a_deferred_index(g):
    """collide_terms_long after its deferral: the similarity re-rank equals sim_ref, and dedup with a
    similarity bound equals join_ref: every key of a colliding pair is 3 edits of 11 characters from
    its partner (similarity 8/11), so a bound of 0.8 keeps them apart and 0.7 joins them."""
    words, rs, wts = CORPORA["collide_terms_long"]
    idx = _build(words, rs, wts, ("w", g))
    oi = OracleIndexG(words, rs, wts, g=g, wide=True)
    try:
        nk = idx.num_keys()
        keys = [idx.key(k) for k in range(nk)]
        kid = {k: i for i, k in enumerate(keys)}
        kt = {hc.text(k): v for k, v in sim_ref.key_terms(words, rs, wts, wide=True).items()}
        assert set(kt) == set(keys)
        queries = keys + [k.lower() for k in keys[:3]] + [keys[0][:-2], keys[1][2:]]
        for thr, lim, ms in [(0.0, 100, 0.0), (0.3, 5, 0.5), (0.0, 100, 0.75)]:
            got = idx.score_batch_sim(queries, thr, lim, ms)
            for q, rows in zip(queries, got):
                base = oi.score(q, thr, lim)
                sims = sim_ref.record_sims([(sim_ref.units(q, True), kt[k]) for k, _ in base], wide=True)
                wk, ws, wv = sim_ref.rerank([k for k, _ in base], [s for _, s in base], list(sims), ms)
                assert [(k, s, np.float32(v)) for k, s, v in rows] == list(zip(wk, ws, wv)), (g, q, thr, lim, ms)

        thr, lim = 0.3, 10
        edges = []
        for a, key in enumerate(keys):
            row = [kid[k] for k, _ in oi.score(key, thr, 0) if kid[k] != a][:lim]
            edges += [(a, b) for b in row]
        sims = sim_ref.record_sims([(sim_ref.units(keys[a], True), kt[keys[b]]) for a, b in edges], wide=True)
        assert idx.dedup(thr, lim) == join_ref.labels(nk, edges)
        fx = hc.load_collisions()
        pairs = [(kid[hc.text(a) + hc.SUFFIX.lower()], kid[hc.text(b) + hc.SUFFIX])
                 for a, b in fx["same_length_before_tail"][:4]]
        for ms, joined in ((0.8, False), (0.7, True)):
            kept = [e for e, v in zip(edges, sims) if not (v < np.float32(ms))]
            want = join_ref.labels(nk, kept)
            assert all((want[a] == want[b]) == joined for a, b in pairs), (ms, want)
            assert idx.dedup(thr, lim, min_similarity=ms) == want, (g, ms)
    finally:
        idx.dispose()


def test_deferred_builds_leave_no_device_memory_behind(capfd):
    """collide_keys_and_terms padded to 2M characters (8 MB of UTF-32: the arena's two blobs alone are
    16 MB), built and disposed 30 times. A build that returned early without freeing its arena would
    cost at least 30 x 16 MB; free memory must stay within 64 MB of its value after the first build."""
    words, rs, wts = CORPORA["collide_keys_and_terms"]
    rng = random.Random(17)
    alpha = "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    filler = ["".join(rng.choices(alpha, k=100)) for _ in range(20000)]
    words = _text(words) + filler
    assert sum(map(len, words)) * 4 >= 8_000_000
    L = _native.lib()
    arr = ssl.WideStringIndex._words(words)  # one conversion for all the builds

    def once():
        h = L.indexW(arr, len(words), rs, None, 2)
        assert h
        assert L.ngsNumKeys(h) == len(words)
        L.disposeW(h)

    os.environ["NGS_BUILD_TIMING"] = "1"
    try:
        capfd.readouterr()
        once()
        _assert_deferred(capfd.readouterr().err, True, "padded corpus")
    finally:
        os.environ.pop("NGS_BUILD_TIMING", None)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(30):
        once()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(f"free after the first build {free0 >> 20} MB, after 30 more {free1 >> 20} MB")
    assert free0 - free1 < 64 << 20, f"{(free0 - free1) >> 20} MB of device memory gone after 30 deferred builds"
