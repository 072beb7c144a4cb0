"""The edit-distance similarity stage on the GPU: ngsSimilarityDevice / ngsRerankDevice on fabricated
result blocks and behind ngsSearchDevice, and scoreBatchSim* / score_batch_sim, against tests/sim_ref.py.
Every comparison is exact: fp32 bits, counts, key order."""
import ctypes as C
import random
import struct
import threading

import numpy as np
import pytest

import sim_ref
from conftest import fixture_weights, fixture_words, load_fixtures
from oracle_py import OracleIndex, OracleIndexG

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0x7FC0FADE  # a NaN pattern no similarity has: cells the kernels must not write keep it
GUARD = 64


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def f32(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def ready():
    """The buffers torch filled on its current stream are complete before a call on another stream reads them."""
    torch.cuda.current_stream().synchronize()


def pack(queries, cs):
    """Raw queries (sequences of ints) -> device bytes and byte offsets in ngsSearchDevice's layout."""
    dt = np.uint8 if cs == 1 else np.uint32
    flat = np.concatenate([np.asarray(q, dtype=dt) for q in queries] + [np.zeros(0, dtype=dt)])
    offs = np.cumsum([0] + [len(q) * cs for q in queries], dtype=np.int64)
    raw = torch.from_numpy(np.frombuffer(flat.tobytes() + bytes(16), dtype=np.uint8).copy()).to(DEV)
    return raw, torch.from_numpy(offs).to(DEV)


def block(counts, keys, stride):
    """counts[n], keys[n][<= stride] -> device counts and key ids at i * stride (the rest 0xEEEEEEEE)."""
    n = len(counts)
    k = np.full((n, stride), 0xEEEEEEEE, dtype=np.uint32)
    for i, row in enumerate(keys):
        k[i, :len(row)] = row
    return (torch.from_numpy(np.asarray(counts, dtype=np.uint32).view(np.int32)).to(DEV),
            torch.from_numpy(k.view(np.int32)).to(DEV))


def similarity(ix, queries, counts, keys, stride, cs=1, stream=None, qbuf=None):
    """ngsSimilarityDevice -> (sims as u32 bits [n][stride], guard cells)."""
    n = len(queries)
    raw, off = qbuf if qbuf is not None else pack(queries, cs)
    dn, dk = block(counts, keys, stride)
    dv = torch.full((n * stride + GUARD,), FILL, dtype=torch.int32, device=DEV)
    s = stream if stream is not None else torch.cuda.current_stream()
    ready()
    ix.similarity_device(raw.data_ptr(), off.data_ptr(), n, stride, dn.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                         s.cuda_stream)
    s.synchronize()
    out = dv.cpu().numpy().view(np.uint32)
    assert np.array_equal(dn.cpu().numpy().view(np.uint32), np.asarray(counts, dtype=np.uint32)), "dCounts written"
    return out[:n * stride].reshape(n, stride), out[n * stride:]


def term_map(ix, words, row_size=1, weights=None, wide=False):
    """key id -> the key's normalised terms, through the key strings of the index."""
    kt = sim_ref.key_terms(words, row_size, weights, wide)
    out = []
    for k in range(ix.num_keys()):
        s = ix.key(k)
        out.append(kt[tuple(sim_ref.units(s, wide))])
    assert len(out) == len(kt)
    return out


def expect(queries, counts, keys, stride, terms, valid=sim_ref.DEFAULT_VALID, wide=False):
    """The block ngsSimilarityDevice must leave: sims where r < min(count, stride), FILL elsewhere."""
    n = len(queries)
    want = np.full((n, stride), FILL, dtype=np.uint32)
    pairs, cells = [], []
    for i, q in enumerate(queries):
        for r in range(min(counts[i], stride)):
            k = int(keys[i][r])
            pairs.append((tuple(q), terms[k] if k < len(terms) else None))
            cells.append((i, r))
    sims = bits(sim_ref.record_sims(pairs, valid, wide))
    for (i, r), b in zip(cells, sims):
        want[i, r] = b
    return want


def check_block(got, guard, want, where):
    assert (guard == FILL).all(), f"{where}: wrote past the block"
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{where}: query {bad[0][0]} record {bad[0][1]}: got "
                           f"{got[tuple(bad[0])]:#x} ({got[tuple(bad[0])].view(np.float32)}), want "
                           f"{want[tuple(bad[0])]:#x} ({want[tuple(bad[0])].view(np.float32)})")


# ---- the short path, narrow ---------------------------------------------------------------
def narrow_words(rng):
    words = []
    for n in (1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 199, 200):  # runs of one letter
        words += [b"A" * n, b"B" * n]
    for _ in range(40):  # equal up to the last character
        base = bytes(rng.choice(b"ABCDE") for _ in range(rng.randint(1, 150)))
        words += [base + b"X", base + b"Y", base]
    for _ in range(60):  # inner spaces
        words.append(b" ".join(bytes(rng.choice(b"ABCDEFG") for _ in range(rng.randint(1, 9))) for _ in range(rng.randint(2, 9))))
    for _ in range(60):  # lower case
        words.append(bytes(rng.choice(b"abcdeXYZ019") for _ in range(rng.randint(1, 120))))
    for _ in range(60):  # bytes outside the validChar set, and >= 0x80
        words.append(b"K" + bytes(rng.choice(b"AB#-_!\x80\xe9\xffcd ") for _ in range(rng.randint(1, 80))) + b"Z")
    for _ in range(120):
        words.append(bytes(rng.choice(b"ABCD") for _ in range(rng.randint(1, 200))))
    return words


def query_of(rng, words, m):
    """A raw query whose normalised length is m: a window of a key (repeated to length) with a few edits,
    lower-cased in places, invalid bytes inside, wrapped in blanks and invalid bytes that the trim removes."""
    src = rng.choice([w for w in words if len(w) >= 2])
    core = bytearray((src * (m // len(src) + 1))[:m])
    for _ in range(max(1, m // 8)):
        core[rng.randrange(m)] = rng.choice(b"ABCDabcd#\x80 E")
    core[0], core[-1] = rng.choice(b"ABcd"), rng.choice(b"XYab")
    return bytes(rng.choice([b"", b" ", b"#\t ", b"\xff - "])) + bytes(core) + bytes(rng.choice([b"", b"  ", b"\n#", b" -\x80"]))


@pytest.fixture(scope="module")
def narrow():
    rng = random.Random(0x51)
    words = narrow_words(rng)
    ix = ssl.StringIndex(words, 1)
    yield ix, words, term_map(ix, words)
    ix.dispose()


def test_short_path_narrow(narrow):
    ix, words, terms = narrow
    rng = random.Random(0x52)
    nk = ix.num_keys()
    assert 380 <= nk <= 470
    stride = 200
    count_set = [0, 1, 15, 16, 17, 63, 64, 65, 130, stride]
    queries, ms = [], []
    for rep in range(2):
        for m in (1, 2, 31, 32, 33, 63, 64):
            q = query_of(rng, words, m)
            assert len(sim_ref.normalise(q)) == m and len(q) >= m
            queries.append(q)
            ms.append(m)
    queries += [b"", b"*", b" \t# ", words[5], words[40].lower()]  # wildcards, nothing left, exact keys
    assert any(len(q) > m for q, m in zip(queries, ms))
    counts = [count_set[(3 * i + 1) % len(count_set)] for i in range(len(queries))]
    counts[queries.index(next(q for q, m in zip(queries, ms) if m == 64))] = stride
    assert set(counts) == set(count_set)
    keys = [[rng.randrange(nk) for _ in range(c)] for c in counts]
    qs = [list(q) for q in queries]
    got, guard = similarity(ix, qs, counts, keys, stride)
    check_block(got, guard, expect(qs, counts, keys, stride, terms), "default set")
    # another validChar set changes Q, not the terms
    other = b"ABCDabcd 019"
    ix.set_valid_char(other)
    try:
        assert any(sim_ref.normalise(q, other) != sim_ref.normalise(q) for q in queries)
        got, guard = similarity(ix, qs, counts, keys, stride)
        check_block(got, guard, expect(qs, counts, keys, stride, terms, valid=other), "after setValidChar")
    finally:
        ix.set_valid_char(sim_ref.DEFAULT_VALID)


# ---- the short path, wide -----------------------------------------------------------------
def colliding_pair():
    """Two characters >= 256 with one home slot in the match-mask table (ngs_sim.h: sim_slot)."""
    slot = lambda c: ((c * 0x9E3779B1) & 0xFFFFFFFF) >> 25
    seen = {}
    for c in range(0x4E00, 0x5000):
        if slot(c) in seen:
            return seen[slot(c)], c
        seen[slot(c)] = c
    raise AssertionError("no collision")


def wide_material():
    rng = random.Random(0x53)
    c1, c2 = colliding_pair()
    alpha = [ord(c) for c in "ABCDabcd 09"] + [0xE9, 0xDF, 0xFF, 0x100, 0x65E5, 0x672C, c1, c2, 0x1F600, 0x20000, 0x10FFFF]
    words = ["".join(chr(rng.choice(alpha)) for _ in range(rng.randint(1, 90))) for _ in range(120)]
    distinct = [0x3041 + i for i in range(64)]  # 64 distinct characters: the table's full load
    words += ["".join(map(chr, distinct)), "".join(map(chr, distinct[:63])) + "A", chr(c1) + chr(c2) * 3 + chr(c1),
              chr(c2) * 5, "日本語テキスト", "Z" * 70]
    queries = [distinct, distinct[::-1], [c1, c2, c1, c1, c2], [c2, c2, c2, c2, c1],
               [32, 0x110000] + [ord(c) for c in "ab日本cd"] + [0xFFFFFFFF, 9],  # trimmed non-code-points
               [ord("Q")] * 7,  # no character of it in most terms
               [ord(c) for c in "日本語テキスト"], [0x1F600, 0x20000, 0xE9, 0xFF, 0x100], [], [ord("*")],
               [rng.choice(alpha) for _ in range(70)], [ord("z")] + [rng.choice(alpha) for _ in range(128)] + [ord("z")]]
    for m in (1, 2, 31, 32, 33, 63):
        src = rng.choice([w for w in words if len(w) >= 2])
        q = [ord(c) for c in (src * (m // len(src) + 1))[:m]]
        q[0] = q[-1] = ord("b")
        queries.append([32, 32] + q + [0x110000])
    return words, queries


def test_short_path_wide():
    words, queries = wide_material()
    rng = random.Random(0x54)
    ix = ssl.WideStringIndex(words, 1, gram_size=2)
    try:
        terms = term_map(ix, words, wide=True)
        nk, stride = ix.num_keys(), 96
        count_set = [0, 1, 15, 16, 17, 63, 64, 65, stride]
        counts = [count_set[(2 * i + 3) % len(count_set)] for i in range(len(queries))]
        counts[0] = counts[2] = stride
        keys = [[rng.randrange(nk) for _ in range(c)] for c in counts]
        keys[0] = list(range(stride))
        got, guard = similarity(ix, queries, counts, keys, stride, cs=4)
        check_block(got, guard, expect(queries, counts, keys, stride, terms, wide=True), "wide")
    finally:
        ix.dispose()


def test_short_path_utf8_handle_behind_the_device_decoder():
    words, queries = wide_material()
    rng = random.Random(0x55)
    enc = lambda q: b"".join(chr(c).encode() if c <= 0x10FFFF else bytes([0xFF]) for c in q)  # 0xFF: an invalid byte
    q8 = [enc(q) for q in queries]
    units = [[c if c <= 0x10FFFF else 0x110000 + 0xFF for c in q] for q in queries]  # what the decoder makes of it
    ix = ssl.Utf8StringIndex(words, 1, gram_size=2)
    try:
        terms = term_map(ix, words, wide=True)
        nk, stride = ix.num_keys(), 70
        counts = [(17 * i + 5) % (stride + 1) for i in range(len(queries))]
        keys = [[rng.randrange(nk) for _ in range(c)] for c in counts]
        raw8, off8 = pack([list(q) for q in q8], 1)
        nbytes = sum(len(q) for q in q8)
        out = torch.zeros(4 * nbytes + 16, dtype=torch.uint8, device=DEV)
        out_off = torch.zeros(len(q8) + 1, dtype=torch.int64, device=DEV)
        s = torch.cuda.Stream()
        ready()
        ssl.utf8_decode_device(raw8.data_ptr(), off8.data_ptr(), len(q8), out.data_ptr(), 4 * nbytes, out_off.data_ptr(),
                               s.cuda_stream)
        got, guard = similarity(ix, units, counts, keys, stride, cs=4, stream=s, qbuf=(out, out_off))
        check_block(got, guard, expect(units, counts, keys, stride, terms, wide=True), "utf-8 handle")
    finally:
        ix.dispose()


# ---- the long path ------------------------------------------------------------------------
def test_long_path():
    rng = random.Random(0x56)
    rs = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    words = [b"A", b"G"]
    for ln in (63, 64, 65, 300):
        words += [rs(ln), rs(ln)]
    queries = {m: rs(m) for m in (65, 127, 128, 129, 1000, 4095, 4096, 4097)}
    for m in (65, 128, 1000, 4096):  # a key equal to the query, and one differing in its last character only
        words += [queries[m], queries[m][:-1] + b"%"]
    words.append(queries[129][:64])  # a key that is the query's first word
    ix = ssl.StringIndex(words, 1)
    try:
        terms = term_map(ix, words)
        nk = ix.num_keys()
        assert nk == len(words)
        qs = [list(b" #" + q.lower() + b"\t") for q in queries.values()]
        counts = [nk] * len(qs)
        keys = [list(range(nk)) for _ in qs]
        got, guard = similarity(ix, qs, counts, keys, nk)
        want = expect(qs, counts, keys, nk, terms)
        check_block(got, guard, want, "long")
        assert (want[-1] == bits([-1.0])[0]).all()  # m = 4,097: not computed
        one = bits([1.0])[0]
        assert sum(int((want[i] == one).sum()) for i in range(len(qs))) == 4  # the equal keys
    finally:
        ix.dispose()


def test_long_path_wide():
    rng = random.Random(0x57)
    alpha = [ord(c) for c in "ABCD"] + [0xE9, 0x65E5, 0x1F600]
    rs = lambda n: [rng.choice(alpha) for _ in range(n)]
    words = [rs(n) for n in (1, 63, 64, 65, 300)]
    queries = [rs(m) for m in (65, 128, 129, 700)]
    words += [queries[0], queries[3][:-1] + [ord("A") if queries[3][-1] != ord("A") else ord("B")]]
    ix = ssl.WideStringIndex(words, 1, gram_size=2)
    try:
        terms = term_map(ix, words, wide=True)
        nk = ix.num_keys()
        qs = [[32] + q + [0x110000] for q in queries]
        counts, keys = [nk] * len(qs), [list(range(nk)) for _ in qs]
        got, guard = similarity(ix, qs, counts, keys, nk, cs=4)
        check_block(got, guard, expect(qs, counts, keys, nk, terms, wide=True), "long wide")
    finally:
        ix.dispose()


# ---- aliases ------------------------------------------------------------------------------
ALIAS_QUERIES = [b"proxima", b"rigil kent", b"alpha centauri", b"visible alias", b"hidden master", b"shared term",
                 b"beta orionis", b"negative", b"only alias", b"zzz", b"solo", b"*"]


def alias_check(words, weights, unique):
    ix = ssl.StringIndex(words, 3, weights)
    try:
        dig = (C.c_uint64 * 17)()
        assert _native.lib().ngsIndexDigest(ix.handle, dig, 17) == 17
        assert (dig[16] & 1) == (1 if unique else 0), "the corpus does not have the shape this case is about"
        terms = term_map(ix, words, 3, weights)
        nk = ix.num_keys()
        qs = [list(q) for q in ALIAS_QUERIES]
        counts, keys = [nk] * len(qs), [list(range(nk)) for _ in qs]
        got, guard = similarity(ix, qs, counts, keys, nk)
        want = expect(qs, counts, keys, nk, terms)
        check_block(got, guard, want, f"aliases unique={unique}")
        return ix.num_keys(), want, [ix.key(k) for k in range(nk)]
    finally:
        ix.dispose()


def test_aliases_keys_with_several_terms():
    words = [b"ALPHA CENTAURI", b"PROXIMA", b"RIGIL KENT",
             b"HIDDEN MASTER", b"VISIBLE ALIAS", None,          # master weight 0: an alias-only key
             b"BETA ORIONIS", b"SHARED TERM", b"RIGEL",
             b"GAMMA CRUCIS", b"SHARED TERM", b"NEGATIVE",      # one term under two keys; negative weights
             b"SOLO", None, None]
    weights = [1.0, 0.5, 2.0, 0.0, 1.0, 1.0, 1.0, 1.0, -1.0, -0.5, 0.25, -2.0, 1.0, 1.0, 1.0]
    nk, want, names = alias_check(words, weights, unique=False)
    assert nk == 5
    one = bits([1.0])[0]
    row = lambda q: dict(zip(names, want[ALIAS_QUERIES.index(q)]))
    assert row(b"proxima")[b"ALPHA CENTAURI"] == one  # matched through the alias: the alias's similarity
    assert row(b"visible alias")[b"HIDDEN MASTER"] == one and row(b"hidden master")[b"HIDDEN MASTER"] != one
    assert row(b"shared term")[b"BETA ORIONIS"] == one and row(b"shared term")[b"GAMMA CRUCIS"] == one
    assert row(b"negative")[b"GAMMA CRUCIS"] == one


def test_aliases_keys_with_one_pair_each():
    words = [b"ALPHA CENTAURI", None, None,
             b"HIDDEN MASTER", b"ONLY ALIAS", None,              # master weight 0: its one pair is the alias
             b"BETA ORIONIS", b"SHARED TERM", None,              # one term under two keys, each key's only pair
             b"GAMMA CRUCIS", b"PROXIMA", b"SHARED TERM",
             b"SOLO", b"RIGIL KENT", b"NEGATIVE"]
    weights = [1.0, 1.0, 1.0, 0.0, -1.5, 1.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.5, 0.0, 0.0, -2.0]
    nk, want, names = alias_check(words, weights, unique=True)
    assert nk == 5
    one = bits([1.0])[0]
    row = lambda q: dict(zip(names, want[ALIAS_QUERIES.index(q)]))
    assert row(b"only alias")[b"HIDDEN MASTER"] == one and row(b"hidden master")[b"HIDDEN MASTER"] != one
    assert row(b"shared term")[b"BETA ORIONIS"] == one and row(b"shared term")[b"GAMMA CRUCIS"] == one
    assert row(b"negative")[b"SOLO"] == one and row(b"solo")[b"SOLO"] != one


# ---- bad input ----------------------------------------------------------------------------
def test_bad_input_has_defined_answers(narrow):
    ix, words, terms = narrow
    nk, stride = ix.num_keys(), 20
    qs = [list(b"abcde"), list(b"AAAA " * 20), list(b"*")]
    keys = [[0, nk, 0xFFFFFFFF, nk - 1, nk + 1] + [3] * 15 for _ in qs]
    counts = [5, stride + 5, stride + 5]  # above the stride: read as the stride
    got, guard = similarity(ix, qs, counts, keys, stride)
    want = expect(qs, counts, keys, stride, terms)
    check_block(got, guard, want, "bad input")
    none = bits([-1.0])[0]
    for i in (0, 1):
        assert want[i][1] == none and want[i][2] == none and want[i][4] == none and want[i][0] != none
    assert (want[1] != FILL).all() and (want[0][5:] == FILL).all()


# ---- re-rank ------------------------------------------------------------------------------
def rerank_case(ix, sims, queries, counts, keys, stride, min_sim, where):
    """ngsRerankDevice on a fabricated block (scores: distinct values) against sim_ref.rerank of `sims`, the
    block's reference similarities (expect)."""
    n = len(queries)
    raw, off = pack(queries, 1)
    dn, dk = block(counts, keys, stride)
    sc = np.arange(n * stride, dtype=np.float32).reshape(n, stride) * np.float32(0.25) + np.float32(1.0)
    ds = torch.from_numpy(sc.copy()).to(DEV)
    dv = torch.full((n * stride + GUARD,), FILL, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    ready()
    ix.rerank_device(raw.data_ptr(), off.data_ptr(), n, stride, dn.data_ptr(), dk.data_ptr(), ds.data_ptr(),
                     dv.data_ptr(), min_sim, s.cuda_stream)
    s.synchronize()
    gn = dn.cpu().numpy().view(np.uint32)
    gk = dk.cpu().numpy().view(np.uint32).reshape(n, stride)
    gs = ds.cpu().numpy().view(np.uint32).reshape(n, stride)
    gv = dv.cpu().numpy().view(np.uint32)
    assert (gv[n * stride:] == FILL).all(), f"{where}: wrote past the block"
    gv = gv[:n * stride].reshape(n, stride)
    for i in range(n):
        c = min(counts[i], stride)
        wk, ws, wv = sim_ref.rerank(list(keys[i][:c]), list(sc[i][:c]), list(sims[i][:c].view(np.float32)), min_sim)
        assert gn[i] == len(wk), f"{where}: query {i} keeps {gn[i]}, want {len(wk)}"
        assert gk[i][:len(wk)].tolist() == [int(k) for k in wk], f"{where}: query {i} key order"
        assert gs[i][:len(wk)].tolist() == bits(ws).tolist(), f"{where}: query {i} scores do not travel with their keys"
        assert gv[i][:len(wk)].tolist() == bits(wv).tolist(), f"{where}: query {i} sims"
        assert sorted(zip(gk[i][:len(wk)].tolist(), gs[i][:len(wk)].tolist())) == sorted(
            (int(k), int(b)) for k, b in zip(wk, bits(ws))), f"{where}: query {i} survivors"


def test_rerank(narrow):
    ix, words, terms = narrow
    rng = random.Random(0x58)
    nk, stride = ix.num_keys(), 4096
    count_set = [0, 1, 64, 65, 1000, 4096]
    queries = [list(query_of(rng, words, m)) for m in (5, 12, 20, 31, 40, 64)]
    queries += [list(b"*"), list(words[30]), list(b"ab")]
    counts = count_set + [300, 64, 200]
    keys = []
    for c in counts:
        row = [rng.randrange(nk) for _ in range(c)]
        for j in range(0, c, 37):
            row[j] = nk + j  # outside the index: sim -1
        keys.append(row)
    keys[7] = [17] * counts[7]  # every record ties: the order stays (one wave)
    keys[8] = [23] * counts[8]  # ... and through the workgroup's sort
    sims = expect(queries, counts, keys, stride, terms)
    pivot = float(sims[4][123].view(np.float32))  # one record's own similarity: it is kept (< drops)
    assert 0.0 < pivot < 1.0
    for ms in (-1.0, 0.0, 0.5, 1.0, pivot):
        rerank_case(ix, sims, queries, counts, keys, stride, ms, f"min {ms}")


def test_rerank_small_stride_and_clamped_count(narrow):
    ix, words, terms = narrow
    rng = random.Random(0x59)
    nk = ix.num_keys()
    for stride in (1, 63, 64, 65, 130):
        queries = [list(query_of(rng, words, 9)) for _ in range(5)]
        counts = [stride + 5, stride, stride // 2, 0, 1]
        keys = [[rng.randrange(nk) for _ in range(min(c, stride))] for c in counts]
        rerank_case(ix, expect(queries, counts, keys, stride, terms), queries, counts, keys, stride, 0.1, f"stride {stride}")


# ---- end to end ---------------------------------------------------------------------------
def sim_expected(answers, queries, terms_by_key, valid, min_sim, wide=False):
    """Oracle answers [(key, score)] per query -> [(key, score bits, sim bits)] after the similarity and the re-rank."""
    pairs = [(tuple(sim_ref.units(q, wide)), terms_by_key[tuple(sim_ref.units(k, wide))]) for q, a in zip(queries, answers) for k, _ in a]
    sims = sim_ref.record_sims(pairs, valid, wide)
    out, o = [], 0
    for a in answers:
        ks, ss, vs = sim_ref.rerank([k for k, _ in a], [s for _, s in a], list(sims[o:o + len(a)]), min_sim)
        out.append([(k, int(bits([s])[0]), int(bits([v])[0])) for k, s, v in zip(ks, ss, vs)])
        o += len(a)
    return out


def as_bits(rows):
    return [[(k, int(bits([s])[0]), int(bits([v])[0])) for k, s, v in r] for r in rows]


@pytest.mark.parametrize("name", ["synth_c1", "mixed"])
def test_end_to_end_on_golden_corpora(name):
    fx = next(f for f in load_fixtures() if f["name"] == name)
    words, weights, rs = fixture_words(fx), fixture_weights(fx), fx["rowSize"]
    wstr = [None if w is None else w.decode("latin-1") for w in words]
    gi, oi = ssl.StringIndex(words, rs, weights), OracleIndex(words, rs, weights)
    wi, ui = ssl.WideStringIndex(wstr, rs, weights, gram_size=3), ssl.Utf8StringIndex(wstr, rs, weights, gram_size=3)
    og = OracleIndexG(wstr, rs, weights, g=3, wide=True)
    try:
        kt = sim_ref.key_terms(words, rs, weights)
        ktw = sim_ref.key_terms(wstr, rs, weights, wide=True)
        valid = sim_ref.DEFAULT_VALID
        for ph in fx["phases"]:
            if ph["validChar"] is not None:
                valid = ph["validChar"].encode("latin-1")
                for x in (gi, oi, wi, ui, og):
                    x.set_valid_char(valid)
            groups = {}
            for c in ph["cases"]:
                groups.setdefault((c["thr"], c["limit"]), []).append(c["q"].encode("latin-1"))
            for (tb, limit), qs in groups.items():
                thr = f32(tb)
                if min(limit or 2 ** 31, gi.num_keys()) > sim_ref.RERANK_MAX_STRIDE:
                    continue
                before = gi.score_batch(qs, thr, limit)
                answers = [oi.score(q, thr, limit) for q in qs]
                for ms in (0.0, 0.4):
                    want = sim_expected(answers, qs, kt, valid, ms)
                    where = f"{name} thr={thr} limit={limit} min={ms}"
                    # the device chain on one stream: search, then re-rank
                    stride = max(1, min(limit or 2 ** 31, gi.num_keys()))
                    raw, off = pack([list(q) for q in qs], 1)
                    n = len(qs)
                    dn = torch.zeros(n, dtype=torch.int32, device=DEV)
                    dk = torch.zeros(n * stride, dtype=torch.int32, device=DEV)
                    ds = torch.zeros(n * stride, dtype=torch.float32, device=DEV)
                    dv = torch.zeros(n * stride, dtype=torch.float32, device=DEV)
                    s = torch.cuda.Stream()
                    ready()
                    gi.search_device(raw.data_ptr(), off.data_ptr(), n, thr, limit, stride, dn.data_ptr(), dk.data_ptr(),
                                     ds.data_ptr(), s.cuda_stream)
                    gi.rerank_device(raw.data_ptr(), off.data_ptr(), n, stride, dn.data_ptr(), dk.data_ptr(), ds.data_ptr(),
                                     dv.data_ptr(), ms, s.cuda_stream)
                    s.synchronize()
                    cn = dn.cpu().numpy()
                    ck = dk.cpu().numpy().view(np.uint32).reshape(n, stride)
                    cs_, cv = ds.cpu().numpy().view(np.uint32).reshape(n, stride), dv.cpu().numpy().view(np.uint32).reshape(n, stride)
                    got = [[(gi.key(int(ck[i][r])), int(cs_[i][r]), int(cv[i][r])) for r in range(cn[i])] for i in range(n)]
                    assert got == want, where + " (device chain)"
                    assert as_bits(gi.score_batch_sim(qs, thr, limit, ms)) == want, where + " (score_batch_sim)"
                    # the wide classes against the generic oracle on the same strings
                    qw = [q.decode("latin-1") for q in qs]
                    wantw = sim_expected([og.score(q, thr, limit) for q in qw], qw, ktw, valid, ms, wide=True)
                    assert as_bits(wi.score_batch_sim(qw, thr, limit, ms)) == wantw, where + " (wide)"
                    assert as_bits(ui.score_batch_sim(qw, thr, limit, ms)) == wantw, where + " (utf-8)"
                after = gi.score_batch(qs, thr, limit)
                assert as_bits([[(k, s, 0.0) for k, s in r] for r in before]) == \
                    as_bits([[(k, s, 0.0) for k, s in r] for r in answers]) == \
                    as_bits([[(k, s, 0.0) for k, s in r] for r in after]), f"{name}: scoreBatch changed"
    finally:
        for x in (gi, wi, ui):
            x.dispose()


# ---- handles ------------------------------------------------------------------------------
def small_block(rng, nk, nq=12, stride=40):
    counts = [(7 * i + 3) % (stride + 1) for i in range(nq)]
    return counts, [[rng.randrange(nk) for _ in range(c)] for c in counts], stride


def test_loaded_index_and_two_replicas(narrow, tmp_path):
    ix, words, terms = narrow
    rng = random.Random(0x5A)
    queries = [list(query_of(rng, words, m)) for m in (3, 9, 17, 33, 64, 70)] * 2
    counts, keys, stride = small_block(rng, ix.num_keys())
    want = expect(queries, counts, keys, stride, terms)
    path = tmp_path / "narrow.idx"
    ix.save(path)
    li = ssl.StringIndex.load(path)
    try:
        assert [li.key(k) for k in range(li.num_keys())] == [ix.key(k) for k in range(ix.num_keys())]
        got, guard = similarity(li, queries, counts, keys, stride)
        check_block(got, guard, want, "loaded index")
    finally:
        li.dispose()
    ri = ssl.StringIndex(words, 1, devices=[0, 0])
    try:
        assert ri.replicas() == 2
        got, guard = similarity(ri, queries, counts, keys, stride)
        check_block(got, guard, want, "two replicas")
        assert as_bits(ri.score_batch_sim([bytes(q) for q in queries], 0.3, 20, 0.2)) == \
            as_bits(ix.score_batch_sim([bytes(q) for q in queries], 0.3, 20, 0.2))
    finally:
        ri.dispose()


def test_four_threads_make_the_first_call_at_once():
    rng = random.Random(0x5B)
    words = narrow_words(rng)
    ix = ssl.StringIndex(words, 1)
    try:
        dig = (C.c_uint64 * 17)()
        assert _native.lib().ngsIndexDigest(ix.handle, dig, 17) == 17 and dig[16] & 1  # the lazy key -> term map
        terms = term_map(ix, words)
        jobs = []
        for t in range(4):
            queries = [list(query_of(rng, words, m)) for m in (4, 16, 33, 64, 66)]
            counts, keys, stride = small_block(rng, ix.num_keys(), nq=len(queries))
            jobs.append((queries, counts, keys, stride))
        results, errors = [None] * 4, []
        gate = threading.Barrier(4)

        def work(t):
            try:
                torch.cuda.set_device(0)
                queries, counts, keys, stride = jobs[t]
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    qbuf = pack(queries, 1)
                s.synchronize()
                gate.wait(timeout=30)
                results[t] = similarity(ix, queries, counts, keys, stride, stream=s, qbuf=qbuf)
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))

        th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for x in th:
            x.start()
        for x in th:
            x.join(timeout=60)
        assert not errors, errors
        for t, (queries, counts, keys, stride) in enumerate(jobs):
            check_block(results[t][0], results[t][1], expect(queries, counts, keys, stride, terms), f"thread {t}")
    finally:
        ix.dispose()


# ---- the limit ----------------------------------------------------------------------------
def test_limit_above_the_rerank_cap():
    L = _native.lib()
    words, _, _ = ssl.synth.gen_corpus(6000, seed=77)
    big = ssl.StringIndex(words, 1)
    small = ssl.StringIndex(words[:100], 1)
    try:
        assert big.num_keys() > 4096 and small.num_keys() <= 100
        qs = [words[3], words[50][:8], b"*"]
        arr = (C.c_char_p * len(qs))(*qs)
        counts = (C.c_uint32 * len(qs))(9, 9, 9)
        res = C.POINTER(C.POINTER(C.c_char))()
        sc, sv = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        L.ngsLastError(1)
        assert L.scoreBatchSim(big.handle, arr, len(qs), 0.0, 5000, 0.0, counts, C.byref(res), C.byref(sc), C.byref(sv)) == 0
        assert L.ngsLastError(1) == 0x10003 and list(counts) == [0, 0, 0] and not res and not sc and not sv
        with pytest.raises(ValueError):
            big.score_batch_sim(qs, 0.0, 5000)
        # the effective limit is min(limit, keys): 100 here
        got = small.score_batch_sim(qs, 0.0, 5000, -1.0)
        assert len(got[2]) == small.num_keys()
        oi = OracleIndex(words[:100], 1)
        kt = sim_ref.key_terms(words[:100], 1)
        want = sim_expected([oi.score(q, 0.0, 5000) for q in qs], qs, kt, sim_ref.DEFAULT_VALID, -1.0)
        assert as_bits(got) == want
        # 4,096 itself is taken
        assert len(big.score_batch_sim([b"*"], 0.0, 4096, 0.0)[0]) == 4096
    finally:
        big.dispose()
        small.dispose()
