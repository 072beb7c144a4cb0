"""ngsLoadIndex refuses an element count the file cannot hold before it allocates for it: a count
of 2^39 after a good header used to reach vector::resize inside an extern "C" call (bad_alloc
through the C ABI ends the process, or terabytes are zeroed). A refused file reaches no device
call, so these run without a GPU. The files are made from constants with tests/index_file.py."""
import os
import struct

import pytest

import index_file
from stringsearchlib_amd import _native


def _load(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return _native.lib().ngsLoadIndex(os.fsencode(str(p)))


def _valid_words():
    valid = [0] * 8
    for c in b".%$ @0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ":
        valid[c >> 5] |= 1 << (c & 31)
    return valid


HEADER = index_file.header(csize=1, gsz=3, n_terms=1, n_short=1, n_keys=1, valid=_valid_words())


def test_helper_header_is_the_documented_one():
    assert len(HEADER) == index_file.HEADER_BYTES == 8 + 9 * 4 + 8 * 4
    assert HEADER[:8] == b"NGSIDX01"
    assert struct.unpack_from("<9I", HEADER, 8) == (1, 3, 0, 6, 9, 3, 1, 1, 1)
    assert index_file.scalar_offset("n_short") == 8 + 7 * 4


def test_count_of_2_to_39_and_nothing_else(tmp_path):
    assert _load(tmp_path, "huge.ngs", HEADER + struct.pack("<Q", 1 << 39)) == 0


def test_count_of_exactly_2_to_40(tmp_path):
    assert _load(tmp_path, "max.ngs", HEADER + struct.pack("<Q", 1 << 40)) == 0
    # ... and as a later, one-byte array's count behind a whole first array
    data = HEADER + index_file.array_bytes("term_off", [0, 2]) + struct.pack("<Q", 1 << 40) + b"AB"
    assert _load(tmp_path, "max_bytes.ngs", data) == 0


@pytest.mark.parametrize("name", [n for n, _, _ in index_file.ARRAYS])
def test_count_one_larger_than_the_data_present(tmp_path, name):
    """Every array in turn ends the file one element short of its count."""
    one_key = {"term_off": [0, 2], "term_bytes": list(b"AB"), "tk_off": [0, 1], "tk": [0, 0x3F800000],
               "key_off": [0, 3], "key_bytes": list(b"ab\0"), "wild_w": [0x3F800000]}
    data = HEADER
    for n, width, _ in index_file.ARRAYS:
        if n == name:
            body = index_file.array_bytes(n, one_key[n])
            count = struct.unpack_from("<Q", body)[0]
            data += struct.pack("<Q", count + 1) + body[8:]
            break
        data += index_file.array_bytes(n, one_key[n])
    assert _load(tmp_path, f"short_{name}.ngs", data) == 0


def test_parse_walks_a_whole_file_and_refuses_a_cut_one():
    data = (HEADER + index_file.array_bytes("term_off", [0, 2]) + index_file.array_bytes("term_bytes", list(b"AB"))
            + index_file.array_bytes("tk_off", [0, 1]) + index_file.array_bytes("tk", [0, 0x3F800000])
            + index_file.array_bytes("key_off", [0, 3]) + index_file.array_bytes("key_bytes", list(b"ab\0"))
            + index_file.array_bytes("wild_w", [0x3F800000]))
    f = index_file.parse(data)
    assert (f.csize, f.gsz, f.n_terms, f.n_short, f.n_keys) == (1, 3, 1, 1, 1)
    assert f.terms() == [b"AB"] and f.keys() == [b"ab"] and f.pairs(0) == [(0, 0x3F800000)]
    assert f.spans["term_bytes"] == (index_file.HEADER_BYTES + 8 + 16 + 8, 2, 1)
    for cut in (len(data) - 1, index_file.HEADER_BYTES + 4, 10):
        with pytest.raises(ValueError):
            index_file.parse(data[:cut])
    with pytest.raises(ValueError):
        index_file.parse(data + b"\0")
