"""Planted inputs for the places where the engine relies on a hash, and plain-Python restatements
of those hashes (ints masked to 64 or 32 bits), so that a test can say where an input lands:

* d_hash (ngs_intern.hip): the interner's 64-bit string hash; collision pairs come from
  tests/golden/collisions/intern_collisions.json (tests/golden/make_golden_collisions.py);
* sketch_cell (ngs_kernels.hip): the u4 count sketch's cell of a long-term id, tier 1a's low bits
  and the full kernel's xor fold;
* U64Map::slot (ngs_index.cpp) and gram_at's probe (ngs_kernels.hip): the gram dictionary;
* the exact tables' home slot (wave_insert_slot, table_insert).

The table geometry is read from ngs_common.h: a change there fails the import loudly instead of
leaving the planted inputs stale. tests/test_hash_cases.py proves on the CPU that every planted
input does what it claims before a GPU test relies on it.
"""
import json
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON_H = os.path.join(ROOT, "stringsearchlib_amd", "csrc", "ngs_common.h")
COLLISIONS = os.path.join(ROOT, "tests", "golden", "collisions", "intern_collisions.json")

M64, M32 = (1 << 64) - 1, (1 << 32) - 1
FNV_OFFSET, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3
GOLDEN64, GOLDEN32 = 0x9E3779B97F4A7C15, 0x9E3779B1
FINAL_MUL = 0xD6E8FEB86659FD93


# ---- geometry from ngs_common.h ----------------------------------------------------------
def _constant(pattern, what, text):
    m = re.search(pattern, text, re.M)
    if not m:
        raise RuntimeError(f"hash_cases: {what} not found in {COMMON_H} (pattern {pattern!r}): the geometry moved, "
                           f"so the planted inputs of tests/hash_cases.py must be looked at again")
    return int(m.group(1))


def read_geometry(text=None):
    if text is None:
        with open(COMMON_H) as f:
            text = f.read()
    return {
        "slot_bits": _constant(r"^#ifndef NGS_SLOT_BITS\s*\n#define NGS_SLOT_BITS (\d+)", "NGS_SLOT_BITS's default", text),
        "full_slot_bits": _constant(r"constexpr int kFullSlotBits = (\d+);", "kFullSlotBits", text),
        "sketch_cap": _constant(r"^#ifndef NGS_SKETCH_CAP\s*\n#define NGS_SKETCH_CAP (\d+)", "NGS_SKETCH_CAP's default", text),
        "cell_bits": _constant(r"constexpr int kSketchCellBits = (\d+);", "kSketchCellBits", text),
    }


GEOM = read_geometry()
SLOT_BITS, FULL_SLOT_BITS = GEOM["slot_bits"], GEOM["full_slot_bits"]
SKETCH_CAP, CELL_BITS = GEOM["sketch_cap"], GEOM["cell_bits"]
CELLS_PER_WORD = 32 // CELL_BITS
LEAN_CELL_BITS = SLOT_BITS + 3        # sketch_cell: TableGeom::kBits + 3
FULL_CELL_BITS = FULL_SLOT_BITS + 3
LEAN_CELLS, FULL_CELLS = 1 << LEAN_CELL_BITS, 1 << FULL_CELL_BITS
CELL_MAX = (1 << CELL_BITS) - 1       # kSketchMax
if CELLS_PER_WORD != 8:
    raise RuntimeError("hash_cases: sketch_cell packs 8 cells per word (kBits + 3); kSketchCellBits is no longer 4")


# ---- the interner's hash -----------------------------------------------------------------
def d_hash(chars):
    """d_hash of a string given as a sequence of character values (bytes or code points)."""
    n = len(chars)
    h = FNV_OFFSET ^ (n * GOLDEN64 & M64)
    for c in chars:
        h = ((h ^ (c & M32)) * FNV_PRIME) & M64
    h ^= h >> 31
    h = (h * FINAL_MUL) & M64
    return h ^ (h >> 29)


VALID = set(b".%$ @0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")


def _space(c):
    return c == 32 or 9 <= c <= 13


def wide_term(chars):
    """A wide word as the index holds its term: escapeBlank, trim, toUpper (k_words)."""
    esc = [(c if c in VALID else 32) if c < 128 else (32 if c > 0x10FFFF else c) for c in chars]
    a, b = 0, len(esc)
    while a < b and _space(esc[a]):
        a += 1
    while b > a and _space(esc[b - 1]):
        b -= 1
    return [c - 32 if 97 <= c <= 122 else c for c in esc[a:b]]


def wide_key(chars):
    """A wide row head as the index holds its key: trimmed of ASCII space only (k_rows)."""
    a, b = 0, len(chars)
    while a < b and chars[a] < 128 and _space(chars[a]):
        a += 1
    while b > a and chars[b - 1] < 128 and _space(chars[b - 1]):
        b -= 1
    return list(chars[a:b])


def load_collisions():
    with open(COLLISIONS) as f:
        return json.load(f)


def text(chars):
    return "".join(map(chr, chars))


# ---- the count sketch --------------------------------------------------------------------
def lean_cell(t):
    """sketch_cell<true>: tier 1a, the low bits of the long-term id."""
    return t & (LEAN_CELLS - 1)


def full_cell(t):
    """sketch_cell<false>: the full kernel's xor fold."""
    return ((t & M32) ^ ((t & M32) >> FULL_CELL_BITS)) & (FULL_CELLS - 1)


def lean_group(x, n=3):
    """n long-term ids of one tier-1a cell: LEAN_CELLS ids apart."""
    return [x + i * LEAN_CELLS for i in range(n)]


def full_group(x, n=3):
    """n long-term ids of one full-kernel cell: x, 16384 + (x ^ 1), 32768 + (x ^ 2)."""
    assert x < FULL_CELLS and n <= FULL_CELLS
    return [i * FULL_CELLS + (x ^ i) for i in range(n)]


# ---- the exact tables --------------------------------------------------------------------
def exact_home(rel, bits):
    """Home slot of a relative term id in an exact-count table of 2^bits words."""
    return ((rel * GOLDEN32) & M32) >> (32 - bits)


# ---- the gram dictionary -----------------------------------------------------------------
def gram_key(chars):
    k = 0
    for c in chars:
        k = (k << 21) | c
    return k


def dict_bits(n_keys):
    """U64Map::init(n_keys + 1), as set_gram_dict calls it."""
    bits = 4
    while (1 << bits) < (n_keys + 1) * 2:
        bits += 1
    return bits


def dict_slot(key, bits):
    """U64Map::slot and gram_at's first probe."""
    return ((key * GOLDEN64) & M64) >> (64 - bits)


def dict_layout(keys):
    """The table set_gram_dict lays out: the keys inserted in ascending order, linear probing,
    wrapping at the end. Returns (bits, table) with None for an empty slot."""
    keys = sorted(set(keys))
    bits = dict_bits(len(keys))
    table = [None] * (1 << bits)
    for k in keys:
        assert (sum(s is not None for s in table) + 1) * 2 <= len(table), "the table would grow"
        i = dict_slot(k, bits)
        while table[i] is not None:
            i = (i + 1) & (len(table) - 1)
        table[i] = k
    return bits, table


def dict_probes(key, bits, table):
    """The slots gram_at reads for `key`, in order, up to the key or the first empty slot."""
    i, seen = dict_slot(key, bits), []
    while True:
        seen.append(i)
        if table[i] is None or table[i] == key:
            return seen
        i = (i + 1) & (len(table) - 1)


def _scalars(start):
    c = start
    while c <= 0x10FFFF:
        if not 0xD800 <= c <= 0xDFFF:
            yield c
        c += 1


def g1_chain():
    """Gram size 1: seven code points >= 0x100 whose home slots in the 16-slot table are 14 or 15 (the
    chain wraps to slot 0), absent code points that home into the chain, and absent ones that home
    onto an empty slot."""
    present, inside, outside = [], [], []
    for c in _scalars(0x100):
        if len(present) < 7 and dict_slot(c, 4) >= 14:
            present.append(c)
        elif len(present) == 7:
            break
    bits, table = dict_layout(present)
    assert bits == 4
    for c in _scalars(present[-1] + 1):
        if table[dict_slot(c, 4)] is not None:
            if len(inside) < 6 and dict_slot(c, 4) not in [dict_slot(x, 4) for x in inside]:
                inside.append(c)
        elif len(outside) < 3:
            outside.append(c)
        if len(inside) == 6 and len(outside) == 3:
            break
    return present, inside, outside


G2_ALPHABET = list(range(0x4E00, 0x4E00 + 200))
G2_BITS, G2_TAIL = 8, 8  # 256 slots; every gram's home is one of the last 8


def g2_chain(seed=5, want=100):
    """Gram size 2: terms (walks over G2_ALPHABET) whose about `want` distinct grams all home into the
    last G2_TAIL of 256 slots, absent grams that home there too, and absent grams that home on an
    empty slot. Returns (terms, grams, inside, outside), grams and absent grams as (c0, c1)."""
    def tail(a, b):
        return dict_slot(gram_key((a, b)), G2_BITS) >= (1 << G2_BITS) - G2_TAIL

    nxt = {a: [b for b in G2_ALPHABET if tail(a, b)] for a in G2_ALPHABET}
    rng = random.Random(seed)
    terms, grams = [], set()
    while len(grams) < want:
        walk = [rng.choice([a for a in G2_ALPHABET if nxt[a]])]
        for _ in range(rng.randint(3, 7)):
            out = nxt[walk[-1]]
            if not out:
                break
            fresh = [b for b in out if (walk[-1], b) not in grams]
            walk.append(rng.choice(fresh or out))
        if len(walk) >= 4 and walk not in terms:
            terms.append(walk)
            grams.update(zip(walk, walk[1:]))
    bits, table = dict_layout([gram_key(g) for g in grams])
    inside, outside = [], []
    for a in G2_ALPHABET:
        for b in G2_ALPHABET[::-1]:
            if (a, b) in grams:
                continue
            if tail(a, b) and len(inside) < 6:
                inside.append((a, b))
            elif table[dict_slot(gram_key((a, b)), bits)] is None and len(outside) < 3:
                outside.append((a, b))
    return terms, sorted(grams), inside, outside


# ---- corpora around the interner's collisions ---------------------------------------------
# Wide libraries (lists of code points) of under 2,000 rows, name -> (words, rowSize, weights).
# Corpora 1-6 make the device build meet two different strings in one equal-hash run of the terms,
# of the keys or of both, and defer to the host build; the control differs from corpus 4 in one
# character per pair and does not.
def _a(s):
    return [ord(c) for c in s]


SUFFIX = "SUFFIX01"  # 8 valid characters: what follows a colliding pair keeps the collision


def _near(s):
    """A string of s's shape that does not collide with its partner: the last character moved by one."""
    return s[:-1] + [s[-1] + 1]


def collision_corpora():
    fx = load_collisions()
    same, diff, triple = fx["same_length"], fx["different_length"], fx["triple"]
    # the length seeds the hash: these heads collide with len(SUFFIX) common characters behind them
    same_t, diff_t = fx["same_length_before_tail"], fx["different_length_before_tail"]
    assert fx["tail"] == len(SUFFIX)
    out = {}

    words = []
    for i, (a, b) in enumerate(same[:4]):
        words += [_a(f"head {2 * i:02d} left"), a, _a(f"head {2 * i + 1:02d} right"), b]
    for i in range(6):
        words += [_a(f"filler {i} key"), _a(f"alias {i}")]
    out["collide_terms_short"] = (words, 2, None)

    # the keys differ in the suffix's case, so only the terms (upper-cased) collide; the first key of
    # each pair, normalised, is its term: a query for it is promoted
    words = []
    for a, b in same_t[:4]:
        words += [a + _a(SUFFIX.lower()), b + _a(SUFFIX)]
    words += [_a(f"other key {i}") for i in range(5)]
    out["collide_terms_long"] = (words, 1, [1.0 + 0.25 * (i % 3) for i in range(len(words))])

    words, wts = [], []
    for i, (a, b) in enumerate(same[:4]):
        words += [a, _a(f"alias {2 * i:02d} of a pair"), b, _a(f"alias {2 * i + 1:02d} of a pair")]
        wts += [0.0, 1.0, 0.0, 1.0]
    for i in range(6):
        words += [_a(f"filler {i} key"), _a(f"alias {i}")]
        wts += [1.0, 1.0]
    out["collide_keys_only"] = (words, 2, wts)

    words = [s for pair in same for s in pair] + [_a(f"filler {i} key") for i in range(7)]
    out["collide_keys_and_terms"] = (words, 1, None)
    out["control_no_collision"] = ([s for a, b in same for s in (a, _near(b))] +
                                   [_a(f"filler {i} key") for i in range(7)], 1, None)

    # lengths 4 and 3 (gram size 2: one long and one short term in a run), bare and with the suffix
    # (both long), as heads (keys and terms) and as aliases (terms alone)
    words = []
    for i, ((a, b), (at, bt)) in enumerate(zip(diff, diff_t)):
        if i % 2 == 0:
            words += [a, _a(f"alias {i} a"), b, _a(f"alias {i} b"), at + _a(SUFFIX), None, bt + _a(SUFFIX), None]
        else:
            words += [_a(f"head {i} a"), a, _a(f"head {i} b"), b, _a(f"head {i} c"), bt + _a(SUFFIX),
                      _a(f"head {i} d"), at + _a(SUFFIX)]
    out["collide_lengths_4_and_3"] = (words, 2, None)

    # A, B, A and B, A, B: the run's head string comes back after its partner, as aliases (terms) and
    # as heads (keys); and three strings of one hash where the fixture has them
    (a1, b1), (a2, b2) = same[4], same[5]
    words, wts = [], []
    for i, s in enumerate([a1, b1, a1, b2, a2, b2]):
        words += [_a(f"row {i}"), s]
        wts += [1.0, 1.0 + i]
    for i, s in enumerate([a2, b2, a2, b1, a1, b1]):
        words += [s, _a(f"alias {i}")]
        wts += [2.0, 0.5 * (i + 1)]
    for i, s in enumerate(triple or []):
        words += [_a(f"of three {i}"), s, s, _a(f"three {i}")]
        wts += [1.0, 3.0, 1.0, 1.0]
    out["collide_run_a_b_a"] = (words, 2, wts)
    return out


DEFERRING = ["collide_terms_short", "collide_terms_long", "collide_keys_only", "collide_keys_and_terms",
             "collide_lengths_4_and_3", "collide_run_a_b_a"]
CONTROL = "control_no_collision"
