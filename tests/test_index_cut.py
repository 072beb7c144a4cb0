"""index._cut: flat result arrays -> one list per query by the counts (no GPU, no library)."""
import ctypes as C

import pytest

from stringsearchlib_amd.index import _cut, _ok

COUNTS = (C.c_uint32 * 3)(0, 2, 1)
KEYS = (C.c_char_p * 3)(b"alpha", b"beta", b"gamma")
SCORES = (C.c_float * 3)(1.5, 0.25, 100.0)
TERMS = (C.c_uint32 * 3)(7, 0xFFFFFFFF, 9)


def test_one_column_gives_lists_of_values():
    assert _cut(COUNTS, 3, 3, KEYS) == [[], [b"alpha", b"beta"], [b"gamma"]]
    assert _cut(COUNTS, 3, 3, (SCORES, lambda x: 2 * x)) == [[], [3.0, 0.5], [200.0]]


def test_two_and_three_columns_give_lists_of_tuples():
    assert _cut(COUNTS, 3, 3, KEYS, SCORES) == [[], [(b"alpha", 1.5), (b"beta", 0.25)], [(b"gamma", 100.0)]]
    name = {7: "seven", 9: "nine"}.get
    assert _cut(COUNTS, 3, 3, (KEYS, bytes.upper), SCORES, (TERMS, name)) == \
        [[], [(b"ALPHA", 1.5, "seven"), (b"BETA", 0.25, None)], [(b"GAMMA", 100.0, "nine")]]


def test_pointers_and_fewer_queries_than_counts():
    """The library's arrays come as pointers; counts has a place even for an empty batch."""
    keys = C.cast(KEYS, C.POINTER(C.c_char_p))
    scores = C.cast(SCORES, C.POINTER(C.c_float))
    assert _cut(COUNTS, 2, 2, keys, scores) == [[], [(b"alpha", 1.5), (b"beta", 0.25)]]
    assert _cut((C.c_uint32 * 1)(), 0, 0, keys, scores) == []


def test_a_total_that_is_not_the_sum_of_the_counts_is_refused():
    for total in (2, 4, 0):
        with pytest.raises(AssertionError):
            _cut(COUNTS, 3, total, KEYS, SCORES)


def test_ok_raises_on_a_non_zero_code_only():
    _ok(0, "ngsSearchDevice")
    with pytest.raises(RuntimeError, match=r"^ngsSearchDevice failed: -3$"):
        _ok(-3, "ngsSearchDevice")
    with pytest.raises(OSError, match=r"^ngsSaveIndex\('x'\) failed: -3$"):
        _ok(-3, "ngsSaveIndex('x')", OSError)
