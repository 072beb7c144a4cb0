"""The build model (tests/build_ref.py) pinned by arrays written out by hand, and the comparison
the GPU test uses (build_ref.compare) shown to report a swapped pair, a weight one ulp off, two
swapped keys, n_short off by one and a wild_w that is the key's last pair's weight, not its
maximum, each with the term or key named. CPU only."""
import build_ref
import index_file

F1 = 0x3F800000  # bits of 1.0f


def bits(w):
    return build_ref.f32_bits(w)


def b(s):
    return tuple(s)


def test_rows_aliases_and_last_weight():
    """rowSize 2. The head is trimmed (not escaped, not upper-cased) into the key; ' ab\\t' and 'ab'
    are one key, 'AB' another, both with the term AB. A NULL head and a blank head yield nothing,
    their aliases included. A NULL alias, a head of weight 0 and an alias that normalises to
    nothing are skipped. '-' inside a term is a blank. The last weight of a pair stays."""
    words = [b" ab\t", b"Hello-World", b"AB", None, None, b"x", b"  ", b"y", b"ab", b"#", b"ab", b"hello world"]
    wts = [1.0, 2.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 3.0, -1.0, 4.0]
    m = build_ref.build(words, 2, wts)
    assert m.keys == [b(b"ab"), b(b"AB")]                      # equal lengths: first row first
    assert m.terms == [b(b"AB"), b(b"HELLO WORLD")] and m.n_short == 1
    assert m.tk_off == [0, 2, 3]
    assert m.tk == [[(0, bits(-1.0)), (1, bits(0.5))], [(0, bits(4.0))]]
    assert m.wild_w == [bits(4.0), bits(0.5)]
    # HEL ELL LLO 'LO ' 'O W' ' WO' WOR ORL RLD
    assert m.gram_mode == 0 and m.n_grams == 9 and m.n_post == 9 and m.post == [0] * 9
    code = lambda s: (s[0] << 14) | (s[1] << 7) | s[2]
    assert m.gram_keys == sorted(code(g) for g in [b"HEL", b"ELL", b"LLO", b"LO ", b"O W", b" WO", b"WOR", b"ORL",
                                                    b"RLD"])


def test_key_from_its_first_row_with_a_pair_and_short_last_row():
    """rowSize 3 over 11 words (the last row has two). 'longer' heads row 0 with zero weights only, so
    the key exists from row 3; 'k' has weight 0 itself but a valid alias; '-' keeps its own empty
    term while the alias '#' (empty too) is skipped; LONGER has exactly 2g characters: long."""
    words = [b"longer", b"a1", b"a2", b"-", b"zz", None, b"k", b"longer", b"#", b"longer", b"K"]
    wts = [0.0, -0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 2.0, 5.0, 1.0, 3.0]
    m = build_ref.build(words, 3, wts)
    assert m.keys == [b(b"-"), b(b"k"), b(b"longer")]
    assert m.terms == [b(b""), b(b"K"), b(b"LONGER")] and m.n_short == 2  # short first, each by first word
    assert m.tk == [[(0, F1)], [(2, bits(3.0))], [(1, bits(2.0)), (2, F1)]]  # pairs by first word
    assert m.wild_w == [F1, bits(2.0), bits(3.0)]
    assert m.n_grams == 4 and m.post == [0, 0, 0, 0]            # LON ONG NGE GER


def test_wide_code_points_gram_size_2():
    """U+2003 is no space (kept at the key's and the term's ends); values above 0x10FFFF are blanks
    in the term and trimmed from its ends; U+E9 and U+10FFFF are kept as they are; 2g - 1 = 3
    characters is short, 2g = 4 is long; keys of g characters at 21 bits each."""
    words = [[0x2003, 0x41, 0x62, 0x20], [0x110000, 0xE9, 0x10FFFF, 0xFFFFFFFF], "abcd", "ab"]
    m = build_ref.build(words, 2, None, g=2, wide=True)
    assert m.keys == [(0x2003, 0x41, 0x62), (0x61, 0x62, 0x63, 0x64)]
    assert m.terms == [(0x2003, 0x41, 0x42), (0xE9, 0x10FFFF), (0x41, 0x42), (0x41, 0x42, 0x43, 0x44)]
    assert m.n_short == 3
    assert m.tk == [[(0, F1)], [(0, F1)], [(1, F1)], [(1, F1)]]
    assert m.gram_mode == 1
    assert m.gram_keys == [(0x41 << 21) | 0x42, (0x42 << 21) | 0x43, (0x43 << 21) | 0x44]
    assert m.gram_off == [0, 1, 2, 3] and m.post == [0, 0, 0] and m.gram_row == [0, 1, 2]


def test_gram_size_1_dictionary_and_lookup_table():
    """g = 1: one character is short, two are long. -0.0 is a zero weight; 1e-45 is not."""
    m = build_ref.build([b"ab", b"a", b"c"], 1, [1.0, 1e-45, -0.0], g=1)
    assert m.keys == [b(b"a"), b(b"ab")]                        # by length
    assert m.terms == [b(b"A"), b(b"AB")] and m.n_short == 1
    assert m.tk == [[(0, 1)], [(1, F1)]] and m.wild_w == [1, F1]
    assert m.gram_keys == [0x41, 0x42] and m.gram_off == [0, 1, 2] and m.post == [0, 0]
    hk, hv, nbits = build_ref.ghash(m)
    # 16 slots; 0x41 * 0x9E3779B97F4A7C15 mod 2^64 has top nibble 2, 0x42's product top nibble 12
    assert nbits == 4 and len(hk) == 16
    want_k, want_v = [2**64 - 1] * 16, [0] * 16
    want_k[2], want_v[2], want_k[12], want_v[12] = 0x41, 0, 0x42, 1
    assert hk == want_k and hv == want_v


def test_raw_high_bytes_and_zero_last_weight():
    """Bytes from 0x80 stay in the key, ends included, and are blanks in the term. A repeat of
    weight 0 leaves the earlier weight; a negative repeat replaces it. A key whose pairs are all
    negative has a negative wild_w."""
    m = build_ref.build([b"\x80x\xff", b"\x80x\xff", b"X", b"X"], 1, [2.0, 0.0, 1.0, -3.0])
    assert m.keys == [b(b"X"), b(b"\x80x\xff")]
    assert m.terms == [b(b"X")] and m.n_short == 1
    assert m.tk == [[(1, bits(2.0)), (0, bits(-3.0))]]
    assert m.wild_w == [bits(-3.0), bits(2.0)]
    assert m.n_grams == 0 and m.post == []


def test_unbuilt_and_nan():
    assert not build_ref.build([b"one"], 1, None).indexed
    assert not build_ref.build([b"one", b"two"], 0, None).indexed
    m = build_ref.build([b"ab", b"ab", b"cd"], 1, [1.0, float("nan"), 2.0])
    assert m.tk[0][0][1] & 0x7FC00000 == 0x7FC00000 and m.nan_keys == {0}  # NaN is not 0: it is the last weight


def test_skip_table_fnv_and_geometry():
    m = build_ref.Model()
    m.lists, m.n_long = [[0, 1, 5], [2]], 6
    assert build_ref.skip_table(m, 2, 3) == [0, 2, 3, 0, 1, 1]
    assert build_ref.skip_table(m, 1, 6) == [0, 3, 0, 1]
    build_ref.check_geometry(m, 2, 3)
    build_ref.check_geometry(m, 4, 2)
    for K, span in [(3, 2), (2, 4), (4, 1)]:
        try:
            build_ref.check_geometry(m, K, span)
        except AssertionError:
            continue
        raise AssertionError((K, span))
    # the digest's FNV-1a-64: offset basis 1469598103934665603 (the library's), prime 2^40 + 0x1B3
    assert build_ref.fnv1a64(b"") == 1469598103934665603
    assert build_ref.fnv1a64(b"a") == ((1469598103934665603 ^ 0x61) * 1099511628211) % 2**64
    assert build_ref.fnv1a64(b"ab") == ((build_ref.fnv1a64(b"a") ^ 0x62) * 1099511628211) % 2**64


# ---- the comparison reports what it must -------------------------------------------------

def _library():
    """Key 'ab' has the pairs (AB, 5) and (HELLO WORLD, 2): its maximum is not its last pair. Term AB
    has two pairs; 'ab' and 'AB' have one length."""
    words = [b"ab", b"hello world", b"AB", b"zz"]
    m = build_ref.build(words, 2, [5.0, 2.0, 0.5, 1.0])
    assert m.keys == [b(b"ab"), b(b"AB")] and m.terms == [b(b"AB"), b(b"ZZ"), b(b"HELLO WORLD")]
    assert m.tk == [[(0, bits(5.0)), (1, bits(0.5))], [(1, F1)], [(0, bits(2.0))]]
    assert m.wild_w == [bits(5.0), F1]
    return m


def _image(m):
    f = index_file.parse(build_ref.file_image(m))
    f.arrays = {k: v.copy() for k, v in f.arrays.items()}  # writable
    f.scalars = dict(f.scalars)
    return f


def test_model_image_round_trips():
    for m in [_library(), build_ref.build([[0x2003, 0x41], "abcd", "ab"], 1, None, g=2, wide=True)]:
        f = _image(m)
        assert build_ref.compare(f, m) == []
        assert [tuple(t) for t in f.terms()] == m.terms and [tuple(k) for k in f.keys()] == m.keys


def _one(f, m, *needles):
    bad = build_ref.compare(f, m, "mutant")
    assert bad, "the mutation went unnoticed"
    assert any(all(n in line for n in needles) for line in bad), bad
    return bad


def test_compare_reports_swapped_pairs():
    m = _library()
    f = _image(m)
    f.arrays["tk"][[0, 1]] = f.arrays["tk"][[1, 0]]
    _one(f, m, "term 0 b'AB'", "pair 0", "b'ab'")


def test_compare_reports_one_ulp():
    m = _library()
    f = _image(m)
    f.arrays["tk"][3, 1] += 1
    _one(f, m, "term 2 b'HELLO WORLD'", "b'ab'", "0x40000001", "0x40000000")


def test_compare_reports_swapped_keys():
    m = _library()
    f = _image(m)
    kb = f.arrays["key_bytes"]
    kb[0:3], kb[3:6] = kb[3:6].copy(), kb[0:3].copy()
    _one(f, m, "key 0 is b'AB'", "b'ab'")


def test_compare_reports_n_short():
    m = _library()
    for d in (-1, 1):
        f = _image(m)
        f.scalars["n_short"] += d
        t = "b'ZZ'" if d < 0 else "b'HELLO WORLD'"
        _one(f, m, f"n_short is {2 + d}", "the model says 2", t)


def test_compare_reports_last_pair_wild_w():
    m = _library()
    f = _image(m)
    f.arrays["wild_w"][0] = bits(2.0)  # the weight of key 0's last pair (HELLO WORLD)
    _one(f, m, "wild_w of key 0 b'ab'", "2.0", "5.0")


def test_compare_skips_wild_w_of_nan_keys_only():
    m = build_ref.build([b"ab", b"ab", b"cd"], 1, [1.0, float("nan"), 2.0])
    f = _image(m)
    f.arrays["wild_w"][0] = 0x7FC00000
    assert build_ref.compare(f, m) == []
    f.arrays["wild_w"][1] += 1
    _one(f, m, "wild_w of key 1 b'cd'")
