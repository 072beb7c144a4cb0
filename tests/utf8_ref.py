"""Reference UTF-8 decoder of the U8 tests: Python's own (include/ngram_search.h: the decoding
rule equals bytes.decode('utf-8', 'surrogateescape') with U+DC80+x read as 0x110000 + 0x80 + x)."""
import itertools
import random

# bytes at every boundary of the well-formed table (lead ranges, second-byte ranges, ASCII)
BOUNDARY_POOL = bytes.fromhex("00417F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5FF")


def ref_units(b: bytes) -> list:
    """The units the library must decode b into."""
    return [0x110000 + 0x80 + (c - 0xDC80) if 0xDC80 <= c <= 0xDCFF else c
            for c in map(ord, bytes(b).decode("utf-8", "surrogateescape"))]


def units_of(s) -> list:
    """A word or query of the U8 tests (str or bytes) as the units the wide API takes."""
    return ref_units(s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8", "surrogateescape"))


def all_two_byte() -> list:
    return [bytes((a, b)) for a in range(256) for b in range(256)]


def pool_four_byte() -> list:
    return [bytes(t) for t in itertools.product(BOUNDARY_POOL, repeat=4)]


def random_strings(n: int, seed: int, max_len: int = 40) -> list:
    """Seeded strings of 0..max_len bytes: a mix of well-formed sequences, boundary bytes and noise."""
    rng = random.Random(seed)
    good = ["A", "z", " ", "é", "ß", "日", "語", "€", "\U0001F600", "\U00020000", "߿", "ࠀ", "￿",
            "\U00010000", "\U0010FFFF"]
    out = []
    for _ in range(n):
        want = rng.randint(0, max_len)
        s = bytearray()
        while len(s) < want:
            k = rng.random()
            if k < 0.5:
                s += rng.choice(good).encode()
            elif k < 0.8:
                s.append(rng.choice(BOUNDARY_POOL))
            else:
                s.append(rng.randrange(256))
        out.append(bytes(s[:want]))  # (the cut truncates sequences at the end of the string)
    return out
