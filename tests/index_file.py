"""Reader and writer of index files (ngsSaveIndex / ngsLoadIndex; the layout is documented above
ngsSaveIndex in ngs_abi.cpp). A plain helper imported by tests.

  "NGSIDX01" | 9 u32 scalars | 8 u32 validChar words | 7 arrays, each a u64 element count
  followed by the elements: term_off u64, term_bytes u8, tk_off u32, tk {u32 key, u32 weight
  bits}, key_off u64, key_bytes u8, wild_w f32

Offsets count characters (csize bytes each); every key ends in one NUL character.
"""
import struct

import numpy as np

MAGIC = b"NGSIDX01"
SCALARS = ["csize", "gsz", "gram_mode", "short_term_len", "short_query_len", "full_scan_len", "n_terms",
           "n_short", "n_keys"]
# (name, element width in bytes, numpy dtype of the parsed array)
ARRAYS = [("term_off", 8, "<u8"), ("term_bytes", 1, "u1"), ("tk_off", 4, "<u4"), ("tk", 8, "<u4"),
          ("key_off", 8, "<u8"), ("key_bytes", 1, "u1"), ("wild_w", 4, "<u4")]
HEADER_BYTES = len(MAGIC) + 4 * len(SCALARS) + 4 * 8


def scalar_offset(name: str) -> int:
    """Byte offset of a header scalar in the file."""
    return len(MAGIC) + 4 * SCALARS.index(name)


class IndexFile:
    """A parsed index file.

    scalars  dict of the nine header words
    valid    the 8 validChar words (bit c of the set = valid[c >> 5] >> (c & 31) & 1)
    arrays   name -> numpy array; tk has shape (n, 2) = (key rank, weight bits), wild_w holds the
             weights' fp32 bit patterns (NaN payloads and the sign of zero survive a comparison)
    spans    name -> (byte offset of the first element, element count, element width)
    """

    def __init__(self, scalars, valid, arrays, spans, size):
        self.scalars, self.valid, self.arrays, self.spans, self.size = scalars, valid, arrays, spans, size

    def __getattr__(self, name):
        if name in SCALARS:
            return self.scalars[name]
        if name in self.arrays:
            return self.arrays[name]
        raise AttributeError(name)

    def _chars(self, name, lo, hi):
        cs = self.scalars["csize"]
        raw = self.arrays[name][lo * cs:hi * cs]
        if cs == 1:
            return bytes(raw)
        return tuple(int(x) for x in np.frombuffer(bytes(raw), dtype="<u4"))

    def term(self, t):
        """Term t: bytes (narrow) or a tuple of code points (wide)."""
        off = self.arrays["term_off"]
        return self._chars("term_bytes", int(off[t]), int(off[t + 1]))

    def terms(self):
        return [self.term(t) for t in range(self.scalars["n_terms"])]

    def key(self, k):
        """Key k without its NUL."""
        off = self.arrays["key_off"]
        return self._chars("key_bytes", int(off[k]), int(off[k + 1]) - 1)

    def keys(self):
        return [self.key(k) for k in range(self.scalars["n_keys"])]

    def pairs(self, t):
        """[(key rank, weight bits)] of term t, in file order."""
        off = self.arrays["tk_off"]
        return [(int(k), int(w)) for k, w in self.arrays["tk"][int(off[t]):int(off[t + 1])]]


def parse(data: bytes) -> IndexFile:
    """Walks the whole file; raises ValueError where the layout does not hold."""
    if len(data) < HEADER_BYTES or data[:8] != MAGIC:
        raise ValueError("not an index file")
    sc = struct.unpack_from("<9I", data, 8)
    valid = list(struct.unpack_from("<8I", data, 8 + 36))
    pos = HEADER_BYTES
    arrays, spans = {}, {}
    for name, width, dtype in ARRAYS:
        if pos + 8 > len(data):
            raise ValueError(f"{name}: no element count")
        (n,) = struct.unpack_from("<Q", data, pos)
        if n * width > len(data) - pos - 8:
            raise ValueError(f"{name}: {n} elements do not fit the file")
        spans[name] = (pos + 8, n, width)
        a = np.frombuffer(data, dtype=dtype, count=n * (2 if name == "tk" else 1), offset=pos + 8)
        arrays[name] = a.reshape(-1, 2) if name == "tk" else a
        pos += 8 + n * width
    if pos != len(data):
        raise ValueError(f"{len(data) - pos} bytes after the last array")
    return IndexFile(dict(zip(SCALARS, sc)), valid, arrays, spans, len(data))


def header(csize=1, gsz=3, n_terms=0, n_short=0, n_keys=0, valid=None, gram_mode=None) -> bytes:
    """The magic, scalars and validChar words of a file, from constants."""
    if gram_mode is None:
        gram_mode = 0 if (csize == 1 and gsz == 3) else 1
    sc = [csize, gsz, gram_mode, 2 * gsz, 3 * gsz, gsz, n_terms, n_short, n_keys]
    return MAGIC + struct.pack("<9I", *sc) + struct.pack("<8I", *(valid or [0] * 8))


def array_bytes(name: str, values, count=None) -> bytes:
    """One array as the file holds it; `count` overrides the element count written before it."""
    width, dtype = next((w, d) for n, w, d in ARRAYS if n == name)
    body = np.asarray(values, dtype=dtype).tobytes()
    assert len(body) % width == 0
    return struct.pack("<Q", len(body) // width if count is None else count) + body


def patch(data: bytes, off: int, fmt: str, val) -> bytes:
    b = bytearray(data)
    struct.pack_into(fmt, b, off, val)
    return bytes(b)
