"""The index build, array by array, against an independent model (tests/build_ref.py).

Every corpus goes through three builds: the device build (ngs_intern.hip + ngs_build.hip),
NGS_HOST_INTERN=1 (host interning, device grams) and NGS_HOST_GRAMS=1 (device interning, host
grams). Each build is saved, the file parsed (tests/index_file.py) and every array compared with
the model field by field; ngsKey / ngsKeyW of every id, getSize and getLibSize are the model's;
the digest's gram words are the model's (dictionary indexes: words 0-7 and 17-19; narrow gram
size 3: postings, lists and the digests of post and skip, since gram_off and gram_row are 16 and
8 MiB there and only compared build against build); the three full digests are equal; and one
score_batch per build at (0.0, 7) and (0.3, 100) equals the oracle. Corpora with +-inf or NaN
weights compare arrays only (such scores have no order).

The corpora sit at the build's edges: word counts around the 256-thread blocks, with and
without skipped words; short last rows; one valid word; one term or key shared by every row;
keys equal only after trimming; keys whose first row yields no pair; 2g - 1 and 2g characters
for every gram size; signed, subnormal, infinite and NaN weights; libraries without any pair;
code points up to 0x10FFFF and values above; one and several skip buckets in both gram modes;
different strings of one 64-bit interner hash among the terms, the keys or both, where the device
build defers to the host build (tests/hash_cases.py).
"""
import ctypes as C
import os
import random

import pytest

import build_ref
import hash_cases
import index_file
import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

pytestmark = pytest.mark.gpu

FLT_MAX = 3.4028234663852886e38
INF, NAN = float("inf"), float("nan")
N3, N2, N1, W1, W2, W3 = ("n", 3), ("n", 2), ("n", 1), ("w", 1), ("w", 2), ("w", 3)
ALL = [N3, N2, N1, W1, W2, W3]
BUILDS = [("device", None), ("host_intern", "NGS_HOST_INTERN"), ("host_grams", "NGS_HOST_GRAMS")]
_U32P = C.POINTER(C.c_uint32)


def _units_at(p):
    u = C.cast(p, _U32P)
    out = []
    while u[len(out)]:
        out.append(u[len(out)])
    return tuple(out)


class _Narrow(ssl.StringIndex):
    _string = staticmethod(lambda p: tuple(C.string_at(p)))


class _Wide(ssl.WideStringIndex):
    """Keys come back as tuples of code units: values above 0x10FFFF stay in a key."""
    _string = staticmethod(_units_at)


# ---- corpora: name -> (factory() -> (words, rowSize, weights), shapes, options) -------------
# words are bytes / None (shared by narrow and wide shapes: a byte is a code point there) or lists
# of code units (wide only). Options: K ("one" / "many": asserted skip-bucket count), arrays_only
# (no search: inf / NaN weights).
CORPORA = {}


def corpus(name, shapes, **opts):
    def deco(fn):
        CORPORA[name] = (fn, shapes, opts)
        return fn
    return deco


def _word(i):
    """Distinct words, two in three short at every gram size above 1 (e.g. b'T7'), one long."""
    return b"T%d" % i if i % 3 else b"TERM%05d" % i


def _sizes(n, skip4):
    return lambda: ([_word(i) for i in range(n)], 1, [0.0 if i % 4 == 3 else 1.0 + (i % 5) for i in range(n)]
                    if skip4 else None)


for _n in (2, 3, 255, 256, 257, 511, 512, 513, 1025):
    corpus(f"size{_n}", [N3, W2], **({"K": "many"} if _n == 1025 else {"K": "one"} if _n <= 3 else {}))(_sizes(_n, False))
    corpus(f"size{_n}_skip4", [N3, N1, W3])(_sizes(_n, True))


@corpus("rows3_7words", [N3, W1, N2])
def _():
    return [_word(i) for i in range(7)], 3, None


@corpus("rows3_770words", [N3, W1])
def _():
    ws = [_word(i // 2) if i % 3 else _word(i) for i in range(770)]  # aliases repeat earlier keys
    return ws, 3, [(-1.5, 0.0, 2.0, 1.0)[i % 4] for i in range(770)]


@corpus("rows5_3words", [N3, N2, W2], K="one")
def _():
    return [b"head word", b"alias one", b"a2"], 5, None


@corpus("one_valid_word_of_600", [N3, W2, N1])
def _():
    return [_word(i) for i in range(600)], 1, [2.5 if i == 431 else 0.0 for i in range(600)]


@corpus("one_valid_row_of_200", [N3, W2])
def _():
    ws = []
    for r in range(200):
        ws += [b"only row", b"its alias", b"x"] if r == 77 else [None if r % 2 else b" \t ", _word(r), b"y"]
    return ws, 3, None


@corpus("run_one_pair_1000", [N3, W2, N1])
def _():
    six = [1.0, 0.5, 2.0, -1.0, 3.0, 0.25]
    return [b"Same Key Here"] * 1000, 1, [six[i % 6] for i in range(1000)]


@corpus("run_one_alias_2000_keys", [N3, W2])
def _():
    ws = []
    for i in range(2000):
        ws += [b"key %d" % i, b"the shared alias"]
    return ws, 2, [1.0 + (i % 7) * 0.25 for i in range(4000)]


@corpus("run_7_keys_2000_rows", [N3, N2, W3])
def _():
    rng = random.Random(11)
    keys = [b"alpha key", b"be", b"gamma-key", b"Delta Key", b"delta key", b"e", b"zeta zeta zeta"]
    return [rng.choice(keys) for _ in range(2000)], 1, [rng.choice([1.0, 0.5, -2.0, 0.0, 3.0]) for _ in range(2000)]


@corpus("repeat_last_zero", ALL, K="one")
def _():
    return [b"pair one", b"pair one", b"pq", b"pq"], 1, [2.0, 0.0, 0.75, -0.0]


@corpus("repeat_last_negative", ALL)
def _():
    return [b"pair one", b"pair one", b"pq", b"pq"], 1, [2.0, -3.0, 0.75, -0.5]


@corpus("keys_trim_case_first_row", ALL)
def _():
    ws = [b"AB", b"x1", b" AB", b"x2", b"AB\t", b"x3", b"\nAB ", b"x4",      # one key, four aliases
          b"ab", None, b"AB", None,                                        # two keys, one term
          b"late key", b"la", b"late key", b"lb",                          # first row: zero weights only
          b"zero head", b"valid alias"]                                    # weight 0, but a valid alias
    wts = [1.0, 1.0, 2.0, 1.0, 3.0, 1.0, 0.5, 1.0, 1.0, 1.0, 4.0, 1.0, 0.0, 0.0, 1.5, 2.5, 0.0, 6.0]
    return ws, 2, wts


@corpus("key_lengths_1_to_300_and_5000", [N3, W2, N1])
def _():
    rng = random.Random(5)
    alpha = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    lens = list(range(1, 301)) + [255, 256, 257, 1, 2, 6, 5] * 3
    rng.shuffle(lens)
    made = {}
    ws = []
    for L in lens:  # a repeated length repeats its key
        made.setdefault(L, bytes(rng.choice(alpha) for _ in range(L)))
        ws += [made[L], None]
    ws += [bytes(rng.choice(alpha) for _ in range(5000)), bytes(rng.choice(alpha) for _ in range(5000))]
    return ws, 2, None


@corpus("long_periodic_terms", ALL)
def _():
    """Terms past the 256 characters one lane scans (ngs_build.hip), nearly every gram a repeat."""
    return [b"AB" * 400, b"short", b"ABC" * 300, b"A" * 700, b"AB" * 128, b"AB" * 128 + b"A", b"BA" * 129], 1, None


@corpus("empty_own_terms", [N3, W1, N2], K="one")
def _():
    return [b"#", b"-", b"_", b"-", b"real"], 1, [1.0, 2.0, 3.0, 0.5, 1.0]


@corpus("high_bytes_at_key_ends", [N3, N2, W2])
def _():
    return [b"\x80mid\xff", b"\xa0mid dle\xa0", b"\xffx\x80", b"mid", b" \xa0 padded \xa0 "], 1, None


def _boundary(g):
    a = b"ABCDEFGHIJ"
    return lambda: ([a[:2 * g - 1], a[:2 * g], a[1:2 * g], a[1:2 * g + 1], a[:g], a[:1]], 1, None)


for _g in (1, 2, 3):
    _sh = [("n", _g), ("w", _g)]
    corpus(f"boundary_g{_g}", _sh)(_boundary(_g))
    corpus(f"short_only_g{_g}", _sh, K="one")(
        lambda g=_g: ([b"ABCDE"[:n] for n in range(1, 2 * g)] + [b"Z", b"#"], 1, None))
    corpus(f"long_only_g{_g}", _sh)(
        lambda g=_g: ([b"ABCDEFGHIJKL"[i:i + 2 * g + i % 3] for i in range(5)], 1, None))
    corpus(f"one_long_among_short_g{_g}", _sh)(
        lambda g=_g: ([b"A", b"B", b"ABCDEFGH"[:2 * g + 1], b"C", b"AB"[:max(1, 2 * g - 1)]], 1, None))
    corpus(f"periodic_g{_g}", _sh)(
        lambda: ([b"AAAAAAAAAA", b"ABABABABAB", b"ABCABCABCABC", b"AAAAAA", b"BABABA", b"CABCAB", b"AB", b"A"] * 3, 1,
                 None))


@corpus("signed_weights", [N3, W2, N1])
def _():
    pool = [-FLT_MAX, -2.0, -1e-45, 0.0, 1e-45, 0.5, -0.0, FLT_MAX]
    ws, wts = [], []
    for i in range(96):
        ws += [b"key%02d" % (i % 24), b"alias %d" % (i % 5)]
        wts += [pool[i % 8], pool[(i * 3 + 1) % 8]]
    ws += [b"all negative", b"an1", b"all negative", b"an2", b"only minus max", None]
    wts += [-2.0, -0.5, -1e-45, -FLT_MAX, -FLT_MAX, 1.0]
    return ws, 2, wts


@corpus("inf_weights", [N3, W2], arrays_only=True)
def _():
    return ([b"plus inf", b"pi", b"minus inf", b"mi", b"both of them", b"pi", b"both of them", b"mi"], 2,
            [INF, 1.0, -INF, 2.0, INF, -INF, -INF, INF])


@corpus("nan_among_500_rows", [N3, W2, N1], arrays_only=True)
def _():
    return [_word(i % 400) for i in range(500)], 1, [NAN if i == 313 else 1.0 + i % 3 for i in range(500)]


@corpus("wide_code_points", [W1, W2, W3])
def _():
    cps = [0x7F, 0x80, 0xE9, 0xA0, 0x2003, 0xFFFF, 0x10000, 0x10FFFF]
    ws = [[c, 0x41, c] for c in cps] + [[0x61, c, 0x62, c, 0x63, c, 0x64] for c in cps]
    ws += [[0x10FFFF] * 3, [0x10FFFF] * 6, [0x10FFFF] * 7, cps, list(reversed(cps)), [0x2003, 0x41, 0x2003]]
    return ws, 1, None


@corpus("wide_above_10ffff", [W1, W2, W3])
def _():
    hi, top = 0x110000, 0xFFFFFFFF
    ws = [[hi, 0x61, 0x62, 0x63, top], [0x61, hi, 0x62, top, 0x63, 0x64, 0x65], [top, top], [hi],
          [0x78, 0x79, 0x7A, 0x7A, 0x79, 0x78], [hi, 0x78, 0x79, 0x7A, 0x7A, 0x79, 0x78, top],
          [0x10FFFF, hi, 0x10FFFF, top, 0x10FFFF, 0x10FFFF, 0x10FFFF, 0x10FFFF]]
    return ws, 1, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]


@corpus("skip_many_buckets", [N3, N2, W1, W2], K="many")
def _():
    rng = random.Random(3)  # four letters: every list is long, so the bucket count follows the lists
    return [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(6, 14))) for _ in range(700)], 1, None


# two different strings of one 64-bit interner hash in one run (tests/hash_cases.py): the device build
# defers to the host build, and every array is still the model's (tests/test_gpu_intern_collision.py
# shows that it deferred)
for _name in hash_cases.DEFERRING:
    corpus(_name, [W2, W3])(lambda n=_name: hash_cases.collision_corpora()[n])


CASES = [(name, shape) for name, (_, shapes, _) in CORPORA.items() for shape in shapes]


# ---- plumbing ---------------------------------------------------------------------------

def _as_shape(words, wide):
    if not wide:
        return words
    return [None if w is None else (list(w) if isinstance(w, (bytes, list)) else w) for w in words]


def _build(words, rs, wts, shape, env):
    kind, g = shape
    cls = _Wide if kind == "w" else _Narrow
    if env:
        os.environ[env] = "1"
    try:
        return cls(words, rs, wts, gram_size=g)
    finally:
        if env:
            os.environ.pop(env, None)


def _digest(idx):
    out = (C.c_uint64 * 20)()
    assert _native.lib().ngsIndexDigest(idx.handle, out, 20) == 20
    short = (C.c_uint64 * 18)()
    assert _native.lib().ngsIndexDigest(idx.handle, short, 17) == 17  # a caller that passes 17 gets 17
    assert list(short) == list(out[:17]) + [0]
    return list(out)


def _oracle(words, rs, wts, shape):
    from oracle_py import OracleIndex, OracleIndexG, lib_g
    kind, g = shape
    if shape == N3:
        oi = OracleIndex(words, rs, wts)
        return oi, lambda q, thr, lim: [(tuple(k), s) for k, s in oi.score(bytes(q), thr, lim)]
    oi = OracleIndexG(words, rs, wts, g=g, wide=kind == "w")

    def score(q, thr, lim):
        cap = max(1, min(lim, oi.n_keys()))
        keys, scores = (C.c_uint32 * cap)(), (C.c_float * cap)()
        qa = (C.c_uint32 * (len(q) + 1))(*[int(c) for c in q], 0)
        n = lib_g().ngog_search(oi.h, C.cast(qa, _U32P), thr, lim, keys, scores, cap)
        out = []
        for k, s in zip(keys[:n], scores[:n]):
            ln = C.c_uint32()
            p = lib_g().ngog_key(oi.h, k, C.byref(ln))
            out.append((tuple(p[:ln.value]), s))
        return out
    return oi, score


def _send(shape, queries):
    """Queries (tuples of character values) as the index class takes them."""
    return [bytes(q) for q in queries] if shape[0] == "n" else [list(q) for q in queries]


def _queries(m):
    ks = [k for k in m.keys if len(k) <= 300]
    picks = ks[:3] + ks[len(ks) // 2:len(ks) // 2 + 2] + ks[-2:]
    lowered = [tuple(c + 32 if 65 <= c <= 90 else c for c in k) for k in picks[:2]]
    return picks + lowered + [(42,), ()]


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{k}{g}" for n, (k, g) in CASES])
def test_build_equals_model(name, shape, tmp_path):
    factory, _, opts = CORPORA[name]
    words, rs, wts = factory()
    wide = shape[0] == "w"
    words = _as_shape(words, wide)
    m = build_ref.build(words, rs, wts, g=shape[1], wide=wide)
    assert m.indexed and m.keys, "the corpus has no pair: it belongs to test_no_pair_at_all"
    queries = _queries(m)
    want = None
    if not opts.get("arrays_only"):
        oi, oscore = _oracle(words, rs, wts, shape)
        assert oi.size() == len(m.terms) and oi.lib_size() == m.n_grams and oi.n_keys() == len(m.keys)
        want = {(thr, lim): [oscore(q, thr, lim) for q in queries] for thr, lim in [(0.0, 7), (0.3, 100)]}
    digests = {}
    for build, env in BUILDS:
        what = f"{name} {shape[0]}{shape[1]} {build}"
        idx = _build(words, rs, wts, shape, env)
        try:
            path = str(tmp_path / f"{build}.ngs")
            idx.save(path)
            with open(path, "rb") as fh:
                f = index_file.parse(fh.read())
            bad = build_ref.compare(f, m, what)
            assert not bad, "\n".join(bad)
            assert f.valid == index_file.parse(build_ref.file_image(m)).valid, what
            assert idx.num_keys() == len(m.keys), what
            for k, key in enumerate(m.keys):
                assert idx.key(k) == key, f"{what}: ngsKey({k}) is {build_ref.show(idx.key(k))}, the model says " \
                                          f"{build_ref.show(key)}"
            assert idx.size() == len(m.terms), f"{what}: getSize {idx.size()}, the model has {len(m.terms)} terms"
            assert idx.lib_size() == m.n_grams, f"{what}: getLibSize {idx.lib_size()}, the model has {m.n_grams} grams"
            d = digests[build] = _digest(idx)
            K, span = d[2], d[7]
            for w, v in build_ref.gram_digest_words(m, K, span).items():
                assert d[w] == v, f"{what}: digest word {w} is {d[w]:#x}, the model says {v:#x} (K {K}, span {span})"
            if m.gram_mode == 0:
                assert d[17:20] == [0, 0, 0], what
            if opts.get("K") == "one":
                assert K == 1, f"{what}: K = {K}"
            if opts.get("K") == "many":
                assert K > 1, f"{what}: K = {K}"
            for (thr, lim), ref in (want or {}).items():
                got = idx.score_batch(_send(shape, queries), thr, lim)
                for q, a, b in zip(queries, got, ref):
                    assert a == b, f"{what}: query {build_ref.show(q)} at ({thr}, {lim}): {a[:4]} vs oracle {b[:4]}"
        finally:
            idx.dispose()
    assert digests["device"] == digests["host_intern"], (name, shape, digests)
    assert digests["device"] == digests["host_grams"], (name, shape, digests)


def test_the_k_options_cover_both_gram_modes():
    """At least one corpus with one skip bucket and one with several, asserted, in each mode."""
    for want in ("one", "many"):
        modes = {(k == "n" and g == 3) for n, (_, shapes, o) in CORPORA.items() if o.get("K") == want
                 for k, g in shapes}
        assert modes == {True, False}, want


@pytest.mark.parametrize("kind", ["zero_weights", "null_heads", "blank_heads"])
@pytest.mark.parametrize("shape", [N3, W2, N1], ids=["n3", "w2", "n1"])
def test_no_pair_at_all(kind, shape):
    """size >= 2 but no pair: the device build defers to the host build; the handle is valid,
    getSize and getLibSize are 0 and every search answers nothing."""
    n = 300
    if kind == "zero_weights":
        words, wts = [_word(i) for i in range(n)], [0.0 if i % 2 else -0.0 for i in range(n)]
    elif kind == "null_heads":
        words, wts = [None if i % 2 == 0 else _word(i) for i in range(n)], None
    else:
        words, wts = [b" \t\n " if i % 2 == 0 else _word(i) for i in range(n)], None
    wide = shape[0] == "w"
    words = _as_shape(words, wide)
    m = build_ref.build(words, 2, wts, g=shape[1], wide=wide)
    assert m.indexed and not m.keys and not m.terms and m.n_grams == 0
    for build, env in BUILDS:
        idx = _build(words, 2, wts, shape, env)
        try:
            assert idx.handle and idx.size() == 0 and idx.lib_size() == 0 and idx.num_keys() == 0, (kind, shape, build)
            qs = [tuple(_word(1)), tuple(b"TERM"), (42,), ()]
            for thr, lim in [(0.0, 7), (0.3, 100)]:
                assert idx.score_batch(_send(shape, qs), thr, lim) == [[], [], [], []], (kind, shape, build)
        finally:
            idx.dispose()
