"""stringsearchlib_amd — MI355X-native n-gram fuzzy search (drop-in for StringSearchLib's DLL).

The product is libngram_search.so (C ABI in include/ngram_search.h); this package is a thin
host-side mirror of the reference interface over it. See DESIGN.md.
"""
from .index import (INT32_MAX, METRICS, NO_MATCH, NO_TERM, IndexSet, StringIndex, Utf8StringIndex,  # noqa: F401
                    WideStringIndex, drop_dead_device, merge_results_device, utf8_decode_device)
from . import _native, synth  # noqa: F401

__all__ = ["StringIndex", "WideStringIndex", "Utf8StringIndex", "utf8_decode_device", "INT32_MAX", "METRICS",
           "NO_TERM", "NO_MATCH", "IndexSet", "merge_results_device", "drop_dead_device"]
