"""Every planted input of tests/hash_cases.py does what it claims, proved on the CPU with the
plain-Python restatements of the engine's hashes, before a GPU test relies on it: the interner's
collision fixture, the term ids that share a sketch cell, the code points and grams whose
dictionary chains wrap, and the geometry read from ngs_common.h.
"""
import pytest

import build_ref
import hash_cases as hc

FX = hc.load_collisions()
PAIRS = FX["same_length"] + FX["different_length"]


def test_geometry_is_read_and_a_missing_constant_is_loud():
    assert hc.GEOM == {"slot_bits": hc.SLOT_BITS, "full_slot_bits": hc.FULL_SLOT_BITS,
                       "sketch_cap": hc.SKETCH_CAP, "cell_bits": hc.CELL_BITS}
    assert hc.LEAN_CELLS == 8 << hc.SLOT_BITS and hc.FULL_CELLS == 8 << hc.FULL_SLOT_BITS
    with open(hc.COMMON_H) as f:
        text = f.read()
    for name in ("#define NGS_SLOT_BITS", "kFullSlotBits =", "#define NGS_SKETCH_CAP", "kSketchCellBits ="):
        assert name in text
        with pytest.raises(RuntimeError, match="not found"):
            hc.read_geometry(text.replace(name, name.replace("S", "Z", 1)))


def test_d_hash_known_values():
    """FNV-1a's offset basis shows through for the empty string; the pair the search was first checked with."""
    h = hc.FNV_OFFSET
    h ^= h >> 31
    h = h * hc.FINAL_MUL & hc.M64
    assert hc.d_hash([]) == h ^ (h >> 29)
    assert hc.d_hash([22660, 28127, 422994]) == hc.d_hash([22714, 28127, 19968])
    assert hc.d_hash([65, 66]) != hc.d_hash([66, 65]) and hc.d_hash([65]) != hc.d_hash([65, 0])


def test_fixture_has_what_the_corpora_need():
    assert len(FX["same_length"]) >= 6 and len(FX["different_length"]) >= 2
    assert all(len(a) == len(b) == 3 for a, b in FX["same_length"])
    assert all({len(a), len(b)} == {3, 4} for a, b in FX["different_length"])
    assert FX["triple"] is not None or FX["triple_note"]
    strings = [tuple(s) for p in FX["same_length"] for s in p]
    assert len(set(strings)) == len(strings), "a string in two pairs would merge their runs"


@pytest.mark.parametrize("group", PAIRS + ([FX["triple"]] if FX["triple"] else []), ids=lambda g: "-".join(map(str, g[0])))
def test_fixture_strings_collide_and_survive(group):
    assert len({hc.d_hash(s) for s in group}) == 1
    assert len({tuple(s) for s in group}) == len(group)
    for s in group:
        assert all(0x100 <= c <= 0x10FFFF and not 0xD800 <= c <= 0xDFFF for c in s)
        assert hc.wide_term(s) == s and hc.wide_key(s) == s
        assert hc.text(s).encode("utf-8").decode("utf-8") == hc.text(s)
    suffixed = [s + hc._a(hc.SUFFIX) for s in group]
    assert len({hc.d_hash(s) for s in suffixed}) == len(group), "the length seeds the hash: a suffix ends the collision"


@pytest.mark.parametrize("pair", FX["same_length_before_tail"] + FX["different_length_before_tail"],
                         ids=lambda g: "-".join(map(str, g[0])))
def test_fixture_heads_collide_before_any_tail(pair):
    """Found under the seeds of the longer lengths: equal states after the heads, so every common tail of
    FX["tail"] characters collides, and the bare heads do not."""
    a, b = pair
    assert a != b and hc.d_hash(a) != hc.d_hash(b)
    for tail in (hc.SUFFIX, hc.SUFFIX.lower(), "01234567", "一" * 8):
        assert len(tail) == FX["tail"] and hc.d_hash(a + hc._a(tail)) == hc.d_hash(b + hc._a(tail))
    assert hc.d_hash(a + hc._a(hc.SUFFIX)) != hc.d_hash(b + hc._a(hc.SUFFIX.lower()))
    for s in (a, b):
        assert all(0x100 <= c <= 0x10FFFF and not 0xD800 <= c <= 0xDFFF for c in s)
        assert hc.wide_term(s + hc._a(hc.SUFFIX)) == s + hc._a(hc.SUFFIX)


def _runs(strings):
    """Equal-hash runs holding more than one distinct string."""
    by = {}
    for s in strings:
        by.setdefault(hc.d_hash(s), set()).add(tuple(s))
    return [v for v in by.values() if len(v) > 1]


@pytest.mark.parametrize("name", hc.DEFERRING + [hc.CONTROL])
def test_corpora_collide_where_they_say(name):
    words, rs, wts = hc.collision_corpora()[name]
    assert len(words) // rs < 2000
    m = build_ref.build(words, rs, wts, g=2, wide=True)
    terms, keys = [list(t) for t in m.terms], [list(k) for k in m.keys]
    assert len({tuple(t) for t in terms}) == len(terms) and len({tuple(k) for k in keys}) == len(keys)
    t_runs, k_runs = _runs(terms), _runs(keys)
    want = {"collide_terms_short": (True, False), "collide_terms_long": (True, False),
            "collide_keys_only": (False, True), "collide_keys_and_terms": (True, True),
            "collide_lengths_4_and_3": (True, True), "collide_run_a_b_a": (True, True),
            hc.CONTROL: (False, False)}[name]
    assert (bool(t_runs), bool(k_runs)) == want, (name, len(t_runs), len(k_runs))
    if name == "collide_lengths_4_and_3":
        assert any(len({len(s) for s in r}) > 1 for r in t_runs) and any(len({len(s) for s in r}) > 1 for r in k_runs)
        assert any({len(s) for s in r} == {3, 4} for r in t_runs), "one short and one long term at gram size 2"
    if name == "collide_terms_long":
        assert all(min(len(s) for s in r) >= 11 for r in t_runs)
    if name == "collide_run_a_b_a":
        # the head of a run (its first word) comes back after its partner, with either string first
        flat_alias = [tuple(w) for w in words[1::2] if w is not None]
        flat_head = [tuple(w) for w in words[0::2] if w is not None]
        for flat in (flat_alias, flat_head):
            found = 0
            for run in _runs([list(w) for w in flat]):
                order = [w for w in flat if w in run]
                found += order[0] == order[2] != order[1] if len(order) >= 3 else 0
            assert found >= 2, "A, B, A with each string of a pair first"


def test_control_differs_from_corpus_4_in_one_character_per_pair():
    c4, ctl = hc.collision_corpora()["collide_keys_and_terms"], hc.collision_corpora()[hc.CONTROL]
    assert len(c4[0]) == len(ctl[0]) and c4[1:] == ctl[1:]
    changed = [(a, b) for a, b in zip(c4[0], ctl[0]) if a != b]
    assert len(changed) == len(FX["same_length"])
    assert all(len(a) == len(b) and a[:-1] == b[:-1] and b[-1] == a[-1] + 1 for a, b in changed)


# ---- sketch cells ---------------------------------------------------------------------------
def test_planted_term_ids_share_cells():
    for x in (0, 5, 7, 8, 4095, 8191 - 64):
        ids = hc.lean_group(x)
        assert len({hc.lean_cell(t) for t in ids}) == 1 and len(set(ids)) == 3
        assert max(ids) < 3 * hc.LEAN_CELLS + 64
        assert hc.lean_cell(ids[0] + 1) == hc.lean_cell(ids[0]) + 1  # the neighbour cell, next nibble
    assert hc.lean_cell(7) % 8 == 7 and hc.lean_cell(7) // 8 == hc.lean_cell(0) // 8  # the word's last cell
    for x in (0, 3, 7, 100, 16383 - 64):
        ids = hc.full_group(x)
        assert len({hc.full_cell(t) for t in ids}) == 1 and len(set(ids)) == 3
        assert ids[1] == hc.FULL_CELLS + (x ^ 1) and ids[2] == 2 * hc.FULL_CELLS + (x ^ 2)
        assert max(ids) < 2 * hc.FULL_CELLS + hc.FULL_CELLS
    # ids one tier-1a table apart do not share a full-kernel cell, and the other way round
    assert hc.full_cell(5) != hc.full_cell(5 + hc.LEAN_CELLS)
    assert hc.lean_cell(hc.full_group(5)[1]) != hc.lean_cell(5)


def test_exact_home_is_the_kernels_formula():
    assert hc.exact_home(1, 10) == 0x9E3779B1 >> 22 and hc.exact_home(1, 11) == 0x9E3779B1 >> 21
    assert hc.exact_home(0, 10) == 0 and all(0 <= hc.exact_home(r, 10) < 1024 for r in range(1, 5000, 7))


# ---- gram dictionary chains -----------------------------------------------------------------
def test_g1_chain_wraps():
    present, inside, outside = hc.g1_chain()
    assert len(present) == 7 and all(c >= 0x100 for c in present + inside + outside)
    assert all(hc.dict_slot(c, 4) in (14, 15) for c in present)
    bits, table = hc.dict_layout(present)
    assert bits == 4 and len(table) == 16
    assert [i for i, k in enumerate(table) if k is not None] == [0, 1, 2, 3, 4, 14, 15]
    assert not set(inside + outside) & set(present)
    for c in present:
        assert table[hc.dict_probes(c, bits, table)[-1]] == c
    assert any(len(hc.dict_probes(c, bits, table)) > 2 and hc.dict_probes(c, bits, table)[-1] < 14 for c in present)
    for c in inside:  # walks occupied slots, then stops at the first empty one
        p = hc.dict_probes(c, bits, table)
        assert len(p) >= 2 and table[p[-1]] is None and all(table[i] is not None for i in p[:-1])
    assert any(14 in hc.dict_probes(c, bits, table) and 0 in hc.dict_probes(c, bits, table) for c in inside), "wraps"
    for c in outside:
        assert hc.dict_probes(c, bits, table) == [hc.dict_slot(c, 4)]


def test_g2_chain_wraps():
    terms, grams, inside, outside = hc.g2_chain()
    assert 64 <= len(grams) <= 127 and abs(len(grams) - 100) <= 10
    assert all(len(t) >= 4 for t in terms)
    assert {g for t in terms for g in zip(t, t[1:])} == set(grams)
    keys = [hc.gram_key(g) for g in grams]
    bits, table = hc.dict_layout(keys)
    assert bits == hc.G2_BITS == 8
    assert all(hc.dict_slot(k, bits) >= 256 - hc.G2_TAIL for k in keys)
    used = [i for i, k in enumerate(table) if k is not None]
    assert used == list(range(len(grams) - hc.G2_TAIL)) + list(range(256 - hc.G2_TAIL, 256)), "one chain, wrapped"
    assert inside and outside
    for g in inside:
        p = hc.dict_probes(hc.gram_key(g), bits, table)
        assert p[0] >= 256 - hc.G2_TAIL and p[-1] == len(grams) - hc.G2_TAIL and 0 in p
    for g in outside:
        assert len(hc.dict_probes(hc.gram_key(g), bits, table)) == 1
