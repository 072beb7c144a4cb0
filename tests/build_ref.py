"""An independent model of the index build, in plain Python. A helper imported by tests.

Written from the reference's constructor row loop and init (nGramSearch.hpp:120-172, :54-108)
and from DESIGN.md §2 (canonicalisations), §5 (key ranks) and §9 (gram sizes, wide strings), not
from the library's host or device build. Everything is kept in dictionaries and Python sorts; no
hashing, no scans, no radix sort.

The rules, as this file understands them:

* size < 2, no words or rowSize 0: nothing is built.
* Rows start at 0, rowSize, 2 rowSize, ...; the last row may be shorter. A row whose head is NULL
  or trims to nothing yields nothing.
* The KEY is the head trimmed by C-locale isspace (space, \\t \\n \\v \\f \\r) on code points below
  128 only; nothing else is changed in it (bytes from 0x80, NBSP, U+2003 stay, also at its ends).
* The TERM of a word is escapeBlank (every character outside the default validChar set becomes a
  blank; narrow: every byte from 0x80 too; wide: code points from 128 are kept, values above
  0x10FFFF become blanks), then the same trim, then ASCII upper-casing. The head's term is taken
  from the key.
* Within a row, in word order: NULL words are skipped; a word of weight 0 (+0 or -0) is skipped; an
  alias whose term is empty is skipped (the head's own empty term is kept). NaN is not 0.
* Every word left gives the pair (term, key) the word's weight: the LAST such word's weight stays.
* A key exists from its first row that has a pair. Key rank: (length in characters, that row).
* Terms exist from their first pair. Term ids: short terms (fewer than 2g characters) first, each
  class in order of first appearance (word index).
* A term's pairs are in order of the first word that gave the pair.
* wild_w of a key: the maximum weight over its pairs (DESIGN.md §2's canonicalisation).

Gram side, from the term list alone: the distinct grams of every long term; narrow g = 3 keys a
gram by 7 bits per byte (c0 << 14 | c1 << 7 | c2, a direct index of 2^21), every other shape by 21
bits per character and ranks the distinct keys ascending (the dictionary: id = rank). post holds
long-term indexes (term id - n_short), ascending within a list; gram_row numbers the non-empty lists
in id order; skip[row][b] is the lower bound of b * span in the row's list and skip[row][K] its
length. K and span are the library's (tuning); check_geometry() holds them to their definition.
"""
import bisect
import struct

DEFAULT_VALID = frozenset(b".%$ @0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")
EMPTY_ROW = 0xFFFFFFFF
_M64 = (1 << 64) - 1


def f32_bits(w) -> int:
    return struct.unpack("<I", struct.pack("<f", w))[0]


def bits_f32(b: int) -> float:
    return struct.unpack("<f", struct.pack("<I", b))[0]


def fnv1a64(data: bytes) -> int:
    h = 1469598103934665603
    for c in data:
        h = ((h ^ c) * 1099511628211) & _M64
    return h


def _le(values, fmt) -> bytes:
    return struct.pack(f"<{len(values)}{fmt}", *values)


def units(word):
    """A word as a tuple of character values up to its NUL: bytes, str, or a sequence of ints."""
    if isinstance(word, str):
        u = [ord(c) for c in word]
    else:
        u = [int(c) & 0xFFFFFFFF for c in word]
    return tuple(u[:u.index(0)] if 0 in u else u)


def _is_space(c):
    return c == 32 or 9 <= c <= 13


def _trim(u):
    a, b = 0, len(u)
    while a < b and _is_space(u[a]):
        a += 1
    while b > a and _is_space(u[b - 1]):
        b -= 1
    return u[a:b]


def normalise(u, wide):
    out = []
    for c in u:
        if c < 128 or not wide:
            c = c if c in DEFAULT_VALID else 32
        elif c > 0x10FFFF:
            c = 32
        out.append(c)
    return tuple(c - 32 if 97 <= c <= 122 else c for c in _trim(tuple(out)))


class Model:
    pass


def build(words, row_size, weights, g=3, wide=False) -> Model:
    """words: list of None / bytes / str / sequences of ints; weights: list of floats or None."""
    m = Model()
    m.g, m.wide, m.csize = g, wide, 4 if wide else 1
    m.gram_mode = 0 if (not wide and g == 3) else 1
    m.indexed = not (len(words) < 2 or row_size == 0)
    key_row = {}     # key -> first row with a pair
    term_word = {}   # term -> first word index
    pair = {}        # (term, key) -> [first word index, weight bits]
    if m.indexed:
        for i in range(0, len(words), row_size):
            if words[i] is None:
                continue
            key = _trim(units(words[i]))
            if not key:
                continue
            for j in range(i, min(i + row_size, len(words))):
                if words[j] is None:
                    continue
                wb = f32_bits(weights[j]) if weights is not None else 0x3F800000
                if wb & 0x7FFFFFFF == 0:
                    continue
                term = normalise(key if j == i else units(words[j]), wide)
                if j != i and not term:
                    continue
                key_row.setdefault(key, i)
                term_word.setdefault(term, j)
                pair.setdefault((term, key), [j, wb])[1] = wb
    keys = sorted(key_row, key=lambda k: (len(k), key_row[k]))
    rank = {k: r for r, k in enumerate(keys)}
    by_word = sorted(term_word, key=term_word.get)
    short = [t for t in by_word if len(t) < 2 * g]
    terms = short + [t for t in by_word if len(t) >= 2 * g]
    per_term = {t: [] for t in terms}
    for (t, k), (j, wb) in sorted(pair.items(), key=lambda kv: kv[1][0]):
        per_term[t].append((rank[k], wb))
    m.keys, m.terms, m.n_short = keys, terms, len(short)
    m.tk = [per_term[t] for t in terms]
    m.tk_off = [0]
    for p in m.tk:
        m.tk_off.append(m.tk_off[-1] + len(p))
    best = {}
    m.nan_keys = set()  # keys that own a NaN pair: their wild_w has no defined value
    for p in m.tk:
        for r, wb in p:
            w = bits_f32(wb)
            if w != w:
                m.nan_keys.add(r)
            elif r not in best or w > best[r]:
                best[r] = w
    m.wild_w = [f32_bits(best.get(r, 0.0)) for r in range(len(keys))]
    _grams(m)
    return m


def gram_key(m, chars):
    k = 0
    for c in chars:
        k = (k << (7 if m.gram_mode == 0 else 21)) | c
    return k


def _grams(m):
    g = m.g
    lists = {}  # gram key -> ascending long-term indexes
    for li, t in enumerate(m.terms[m.n_short:]):
        for k in sorted({gram_key(m, t[i:i + g]) for i in range(len(t) - g + 1)}):
            lists.setdefault(k, []).append(li)
    m.n_long = len(m.terms) - m.n_short
    m.gram_keys = sorted(lists)                      # non-empty lists in id order
    m.lists = [lists[k] for k in m.gram_keys]
    m.n_grams = len(m.gram_keys)                     # getLibSize
    m.n_post = sum(len(p) for p in m.lists)
    m.post = [x for p in m.lists for x in p]
    m.G = (1 << 21) if m.gram_mode == 0 else m.n_grams
    if m.gram_mode == 1:                             # every dictionary id has a list
        m.gram_off = [0]
        for p in m.lists:
            m.gram_off.append(m.gram_off[-1] + len(p))
        m.gram_row = list(range(m.n_grams))


def skip_table(m, K, span):
    out = []
    for p in m.lists:
        for b in range(K):
            out.append(bisect.bisect_left(p, b * span))  # the list ascends
        out.append(len(p))
    return out


def check_geometry(m, K, span):
    assert K >= 1 and K & (K - 1) == 0, f"K = {K} is not a power of two"
    want = -(-m.n_long // K) if m.n_long else 1
    assert span == want, f"span {span}, but ceil({m.n_long} / {K}) = {want}"


def ghash(m):
    """Dictionary mode: the lookup table the kernels probe, a function of the key set alone
    (ngs_index.h): 2^bits slots, bits the smallest >= 4 with 2^bits >= 2 (G + 1); the keys inserted
    ascending at slot (key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - bits), linear probing; an empty
    slot holds key ~0 and value 0; the value is the gram id."""
    bits = 4
    while (1 << bits) < 2 * (len(m.gram_keys) + 1):
        bits += 1
    key = [_M64] * (1 << bits)
    val = [0] * (1 << bits)
    for gid, k in enumerate(m.gram_keys):
        i = ((k * 0x9E3779B97F4A7C15) & _M64) >> (64 - bits)
        while key[i] != _M64:
            i = (i + 1) & ((1 << bits) - 1)
        key[i], val[i] = k, gid
    return key, val, bits


def gram_digest_words(m, K, span):
    """The digest words the model can state: {word index: value}. Dictionary mode: 0-7 and 17-19;
    narrow g = 3: 0, 1, 4 and 6 (gram_off and gram_row span 2^21 entries there)."""
    check_geometry(m, K, span)
    out = {0: m.n_post, 1: m.n_grams, 4: fnv1a64(_le(m.post, "I")), 6: fnv1a64(_le(skip_table(m, K, span), "I"))}
    if m.gram_mode == 1:
        hk, hv, bits = ghash(m)
        out.update({2: K, 7: span, 3: fnv1a64(_le(m.gram_off, "Q")), 5: fnv1a64(_le(m.gram_row, "I")),
                    17: fnv1a64(_le(hk, "Q")), 18: fnv1a64(_le(hv, "I")), 19: bits})
    return out


def show(chars):
    """A term or key for a failure message."""
    if isinstance(chars, bytes):
        return repr(chars)
    if all(c < 256 for c in chars):
        return repr(bytes(chars))
    return "[" + " ".join(f"{c:X}" for c in chars) + "]"


def file_image(m) -> bytes:
    """The model as an index file (index_file.py's layout), so a model can be parsed like a save."""
    import index_file
    fmt = "I" if m.wide else "B"
    term_off, key_off = [0], [0]
    tb, kb = b"", b""
    for t in m.terms:
        term_off.append(term_off[-1] + len(t))
        tb += _le(t, fmt)
    for k in m.keys:
        key_off.append(key_off[-1] + len(k) + 1)
        kb += _le(k + (0,), fmt)
    valid = [0] * 8
    for c in DEFAULT_VALID:
        valid[c >> 5] |= 1 << (c & 31)
    tk = [x for p in m.tk for kw in p for x in kw]
    return (index_file.header(m.csize, m.g, len(m.terms), m.n_short, len(m.keys), valid)
            + index_file.array_bytes("term_off", term_off) + index_file.array_bytes("term_bytes", list(tb))
            + index_file.array_bytes("tk_off", m.tk_off) + index_file.array_bytes("tk", tk)
            + index_file.array_bytes("key_off", key_off) + index_file.array_bytes("key_bytes", list(kb))
            + index_file.array_bytes("wild_w", m.wild_w))


def compare(f, m, what="index"):
    """Field by field: the parsed file `f` (index_file.IndexFile) against the model. Returns the
    list of differences, each naming the term or key concerned (at most a few per field)."""
    bad = []

    def say(msg):
        if len(bad) < 12:
            bad.append(f"{what}: {msg}")

    for name, want in [("csize", m.csize), ("gsz", m.g), ("gram_mode", m.gram_mode), ("short_term_len", 2 * m.g),
                       ("short_query_len", 3 * m.g), ("full_scan_len", m.g)]:
        if f.scalars[name] != want:
            say(f"{name} is {f.scalars[name]}, the model says {want}")
    got_terms = [tuple(t) for t in f.terms()]
    got_keys = [tuple(k) for k in f.keys()]
    if f.n_short != m.n_short:
        t = m.terms[min(f.n_short, m.n_short)] if m.terms else ()
        say(f"n_short is {f.n_short}, the model says {m.n_short} (first term classed differently: "
            f"term {min(f.n_short, m.n_short)} {show(t)}, {len(t)} characters)")
    if len(got_terms) != len(m.terms):
        extra = set(got_terms) ^ set(m.terms)
        say(f"{len(got_terms)} terms, the model has {len(m.terms)}; "
            f"on one side only: {[show(t) for t in sorted(extra)[:3]]}")
    for i, (a, b) in enumerate(zip(got_terms, m.terms)):
        if a != b:
            say(f"term {i} is {show(a)}, the model says {show(b)}")
            break
    if len(got_keys) != len(m.keys):
        extra = set(got_keys) ^ set(m.keys)
        say(f"{len(got_keys)} keys, the model has {len(m.keys)}; "
            f"on one side only: {[show(k) for k in sorted(extra)[:3]]}")
    for i, (a, b) in enumerate(zip(got_keys, m.keys)):
        if a != b:
            say(f"key {i} is {show(a)}, the model says {show(b)}")
            break
    if len(got_terms) == len(m.terms):
        if [int(x) for x in f.tk_off] != m.tk_off:
            t = next(i for i, (a, b) in enumerate(zip(f.tk_off[1:], m.tk_off[1:])) if int(a) != b)
            say(f"term {t} {show(m.terms[t])} has {int(f.tk_off[t + 1]) - int(f.tk_off[t])} pairs, "
                f"the model says {len(m.tk[t])}")
        else:
            for t, want in enumerate(m.tk):
                got = f.pairs(t)
                if got == want:
                    continue
                i = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
                (gk, gw), (wk, ww) = got[i], want[i]
                if gk != wk:
                    say(f"term {t} {show(m.terms[t])} pair {i} is key {gk} "
                        f"{show(got_keys[gk]) if gk < len(got_keys) else '?'}, the model says key {wk} "
                        f"{show(m.keys[wk])}")
                else:
                    say(f"term {t} {show(m.terms[t])} pair {i} (key {wk} {show(m.keys[wk])}) has weight bits "
                        f"{gw:#010x} ({bits_f32(gw)!r}), the model says {ww:#010x} ({bits_f32(ww)!r})")
    if len(got_keys) == len(m.keys):
        for k, (a, b) in enumerate(zip(f.wild_w, m.wild_w)):
            if int(a) != b and k not in m.nan_keys:
                say(f"wild_w of key {k} {show(m.keys[k])} is {int(a):#010x} ({bits_f32(int(a))!r}), the model "
                    f"says {b:#010x} ({bits_f32(b)!r}), the maximum of its pairs")
    return bad
