"""ctypes binding of libngram_search.so (include/ngram_search.h).

The library is built in-tree (``make -C stringsearchlib_amd/csrc``) and loaded from
``stringsearchlib_amd/lib``. There is no pure-Python or CPU fallback: if the library is
missing or no GPU is usable the calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import glob
import hashlib
import os
import re
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB_DIR = os.path.join(PKG, "lib")
# NGS_LIB=prof selects the phase-stamped diagnostic build (make -C csrc prof); NGS_LIB=<name>
# selects lib/libngram_search_<name>.so (experiment builds)
_variant = os.environ.get("NGS_LIB", "")
LIB_PATH = os.path.join(LIB_DIR, f"libngram_search_{_variant}.so" if _variant else "libngram_search.so")
SYNTH_PATH = os.path.join(LIB_DIR, "libngs_synth.so")
HEADER = os.path.join(ROOT, "include", "ngram_search.h")
CSRC = os.path.join(PKG, "csrc")


class NgsStats(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("fast_queries", C.c_uint64), ("general_queries", C.c_uint64),
                ("postings", C.c_uint64), ("lists", C.c_uint64), ("results", C.c_uint64), ("survivors", C.c_uint64),
                ("fast_kernel_ms", C.c_double), ("prep_kernel_ms", C.c_double), ("general_ms", C.c_double),
                ("handover_queries", C.c_uint64), ("tier2_queries", C.c_uint64),
                ("heavy_queries", C.c_uint64), ("full_queries", C.c_uint64),
                ("slot_full_queries", C.c_uint64), ("survivor_slots", C.c_uint64),
                ("survivor_slot_bytes", C.c_uint64), ("main_postings", C.c_uint64), ("main_lists", C.c_uint64),
                ("arena_blocks", C.c_uint64), ("arena_used", C.c_uint64)]


class MergePart(C.Structure):
    """ngs_merge_part: one part of ngsMergeResultsDevice (device addresses as integers)."""
    _fields_ = [("dCounts", C.c_void_p), ("dKeys", C.c_void_p), ("dScores", C.c_void_p),
                ("stride", C.c_uint32), ("keyBase", C.c_uint32), ("dKeyLen", C.c_void_p), ("nKeys", C.c_uint32)]


def build(jobs: int = 4) -> None:
    """Compile the HIP library for gfx950 in-tree."""
    subprocess.run(["make", "-s", f"-j{jobs}", "-C", CSRC], check=True)


_lib = None
_synth = None


def source_hash() -> str:
    """The stamp the Makefile bakes into ngsVersion(): SHA-256 (16 hex digits) of the library's
    sources (csrc/*.h, *.hip, *.cpp in byte order, then include/ngram_search.h)."""
    files = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")) +
                   glob.glob(os.path.join(CSRC, "*.cpp"))) + [HEADER]
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


# ---- the exports' signatures (include/ngram_search.h) ----
u32, u64, f32, cp, vp, ci = C.c_uint32, C.c_uint64, C.c_float, C.c_char_p, C.c_void_p, C.c_int
P = C.POINTER
PP = P(P(C.c_char))      # char**: narrow and UTF-8 results
W = P(C.c_uint32)        # wchar_t*: 4 bytes on Linux, bound as uint32 units
PW = P(W)
PF, PT, PU = P(P(f32)), P(P(u32)), P(u32)
# a call that exists per string width: suffix -> (a string, a results array); UTF-8 is char* on a wide index
_WIDTHS = {"": (cp, PP), "W": (W, PW), "U8": (cp, PP)}
STR, STRS, RES = "a string", "an array of strings", "the address of a results array"


def _by_width(widths, rows):
    """{name + suffix: (restype, argtypes)} for every suffix of `widths`, STR / STRS / RES filled in."""
    out = {}
    for w in widths:
        s, r = _WIDTHS[w]
        fill = {STR: s, STRS: P(s), RES: P(r)}
        for name, (restype, argtypes) in rows.items():
            out[name + w] = (restype, [fill.get(a, a) for a in argtypes])
    return out


_QUERY = {"search": (u32, [u32, STR, RES, f32, u32]),
          "score": (u32, [u32, STR, RES, PF, f32, u32]),
          "scoreBatch": (u32, [u32, STRS, u32, f32, u32, PU, RES, PF]),
          "searchBatch": (u32, [u32, STRS, u32, f32, u32, PU, RES])}
_SEARCH_DEVICE = (ci, [u32, vp, vp, u32, f32, u32, u32, vp, vp, vp, vp])
# [(probe, {name: (restype, argtypes)})]: a group whose probe symbol the library lacks is skipped
# (NGS_LIB experiment builds of older sources); probe None: every library has them
EXPORTS = [
    (None, {"indexN": (u32, [P(cp), u64, C.c_uint16, P(f32)]),
            "release": (None, [u32, PP, P(f32)]),
            "dispose": (None, [u32]),
            "getSize": (u64, [u32]),
            "getLibSize": (u64, [u32]),
            "setValidChar": (None, [u32, cp, ci]),
            **_by_width(("", "W"), _QUERY),
            # wide / gram-size extensions
            "indexG": (u32, [P(cp), u64, C.c_uint16, P(f32), C.c_uint16]),
            "indexW": (u32, [P(W), u64, C.c_uint16, P(f32), C.c_uint16]),
            "releaseW": (None, [u32, PW, P(f32)]),
            "disposeW": (None, [u32]),
            "getSizeW": (u64, [u32]),
            "getLibSizeW": (u64, [u32]),
            "ngsKeyW": (vp, [u32, u32]),
            "ngsCharSize": (u32, [u32]),
            "ngsGramSize": (u32, [u32]),
            "ngsSetDevice": (ci, [ci]),
            "ngsSetDevices": (ci, [P(ci), ci]),
            "ngsReplicaCount": (ci, [u32]),
            "ngsDeviceCount": (ci, []),
            "ngsNumKeys": (u32, [u32]),
            "ngsKey": (vp, [u32, u32]),
            "ngsSearchDevice": _SEARCH_DEVICE,
            "ngsSetTiming": (ci, [u32, ci]),
            "ngsLastStats": (ci, [u32, P(NgsStats)]),
            "ngsIndexDigest": (ci, [u32, P(u64), ci]),
            "ngsVersion": (cp, []),
            "ngsSaveIndex": (ci, [u32, cp]),
            "ngsLoadIndex": (u32, [cp]),
            "ngsHostPhases": (ci, [P(u64), ci, ci]),
            "ngsPhaseStats": (ci, [P(u64), ci, ci])}),
    # UTF-8 on wide indexes: strings in and out are char*, the index underneath is the wide one
    ("indexU8", {"indexU8": (u32, [P(cp), u64, C.c_uint16, P(f32), C.c_uint16]),
                 **_by_width(("U8",), _QUERY),
                 "ngsKeyU8": (vp, [u32, u32]),
                 "ngsUtf8Decode": (ci, [vp, vp, u32, vp, u64, vp, vp]),
                 "ngsSearchDeviceU8": _SEARCH_DEVICE}),
    ("ngsSearchDeviceAsync", {"ngsSearchDeviceAsync": (ci, _SEARCH_DEVICE[1] + [P(u64)]),
                              "ngsSearchDeviceWait": (ci, [u32, u64])}),
    ("ngsServe", {"ngsServe": (ci, [u32, ci])}),
    ("ngsPackResults", {"ngsPackResults": (ci, [vp, vp, vp, u32, u32, vp, vp, vp])}),
    # the similarity stage
    ("ngsSimilarityDevice", {"ngsSimilarityDevice": (ci, [u32, vp, vp, u32, u32, vp, vp, vp, vp]),
                             "ngsRerankDevice": (ci, [u32, vp, vp, u32, u32, vp, vp, vp, vp, f32, vp]),
                             **_by_width(("", "W", "U8"), {
                                 "scoreBatchSim": (u32, [u32, STRS, u32, f32, u32, f32, PU, RES, PF, PF])})}),
    # ... by metric, with the matched term
    ("ngsSimilarityDeviceM", {"ngsSimilarityDeviceM": (ci, [u32, vp, vp, u32, u32, vp, vp, u32, vp, vp, vp]),
                              "ngsRerankDeviceM": (ci, [u32, vp, vp, u32, u32, vp, vp, vp, vp, vp, u32, f32, vp]),
                              **_by_width(("", "W", "U8"), {
                                  "scoreBatchSimM": (u32, [u32, STRS, u32, f32, u32, u32, f32, PU, RES, PF, PF, PT])}),
                              "ngsReleaseTerms": (None, [PU]),
                              "dedupKeysM": (u32, [u32, f32, u32, u32, f32, u32, PU]),
                              "ngsTerm": (C.c_int64, [u32, u32, vp, u64])}),
    # the token sort in front of the similarity
    ("ngsTokenSortDevice", {"ngsTokenSortDevice": (ci, [u32, vp, vp, u32, vp, vp])}),
    # the self-join
    ("ngsSelfJoinDevice", {"ngsKeyQueryBytes": (u64, [u32, u32, u32]),
                           "ngsKeyQueriesDevice": (ci, [u32, u32, u32, vp, u64, vp, vp]),
                           "ngsDropSelfDevice": (ci, [vp, vp, vp, u32, u32, u32, u32, vp]),
                           "ngsSelfJoinDevice": (ci, [u32, u32, u32, f32, u32, u32, vp, vp, vp, vp]),
                           "ngsClusterDevice": (ci, [vp, vp, u32, u32, u32, vp, u32, u32, vp]),
                           "selfJoin": (u32, [u32, u32, u32, f32, u32, u32, PU, PU, P(f32)]),
                           "dedupKeys": (u32, [u32, f32, u32, f32, u32, PU])}),
    # linking two indexes
    ("ngsMatchDevice", {"ngsMatchDevice": (ci, [vp, vp, vp, u32, u32, u32, vp, u32, vp, u32, vp, vp, u32, vp]),
                        "linkKeys": (u32, [u32, u32, f32, u32, u32, f32, u32, u32, PU, P(f32), P(f32)])}),
    # index sets
    ("ngsMergeResultsDevice", {"ngsKeyLengthsDevice": (ci, [u32, u32, u32, vp, vp]),
                               "ngsMergeResultsDevice": (ci, [P(MergePart), u32, u32, u32, u32, vp, vp, vp, vp]),
                               "ngsSetCreate": (u32, [PU, u32]),
                               "ngsSetAdd": (ci, [u32, u32]),
                               "ngsSetDispose": (None, [u32]),
                               "ngsSetParts": (ci, [u32]),
                               "ngsSetNumKeys": (u32, [u32]),
                               "ngsSetLocate": (ci, [u32, u32, PU, PU]),
                               "ngsSetSearchDevice": _SEARCH_DEVICE,
                               **_by_width(("", "W", "U8"), {
                                   "scoreBatchSet": (u32, [u32, STRS, u32, f32, u32, u32, PU, PU, P(f32)])})}),
    # the later stages over a set
    ("ngsSetSimilarityDeviceM", {
        "ngsSetSimilarityDeviceM": (ci, [u32, vp, vp, u32, u32, vp, vp, u32, vp, vp, vp]),
        "ngsSetRerankDeviceM": (ci, [u32, vp, vp, u32, u32, vp, vp, vp, vp, vp, u32, f32, vp]),
        "ngsSetKeyQueryBytes": (u64, [u32, u32, u32]),
        "ngsSetKeyQueriesDevice": (ci, [u32, u32, u32, vp, u64, vp, vp]),
        "ngsSetSelfJoinDevice": (ci, [u32, u32, u32, f32, u32, u32, vp, vp, vp, vp]),
        **_by_width(("", "W", "U8"), {
            "scoreBatchSetSimM": (u32, [u32, STRS, u32, f32, u32, u32, f32, u32, PU, PU, P(f32), P(f32), PU])}),
        "selfJoinSet": (u32, [u32, u32, u32, f32, u32, u32, PU, PU, P(f32)]),
        "dedupKeysSet": (u32, [u32, f32, u32, u32, f32, u32, PU])}),
    # dead keys: delete from a set without a rebuild
    ("ngsDropDeadDevice", {"ngsDropDeadDevice": (ci, [vp, vp, vp, u32, u32, vp, u32, u32, vp, vp]),
                           "ngsSetRemove": (ci, [u32, PU, u32]),
                           "ngsSetRestore": (ci, [u32, PU, u32]),
                           "ngsSetLiveKeys": (u32, [u32]),
                           "ngsSetDeadKeys": (u32, [u32, PU, u32]),
                           "ngsSetIsLive": (ci, [u32, u32]),
                           "ngsSetDeadStats": (ci, [u32, P(u64), ci])}),
    ("ngsServeState", {"ngsServeState": (ci, [u32])}),
    ("ngsLastError", {"ngsLastError": (ci, [ci])}),
    ("ngsReplicaDigest", {"ngsReplicaDigest": (ci, [u32, ci, P(u64), ci])}),
]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (HIP, gfx950)")
    L = C.CDLL(LIB_PATH)
    for probe, group in EXPORTS:
        if probe is None or hasattr(L, probe):
            for name, (restype, argtypes) in group.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
    version = L.ngsVersion().decode()
    want = source_hash()
    if not version.endswith(f"src={want}") and _variant:  # experiment builds (NGS_LIB) may predate the tree
        import sys
        print(f"[ngram_search] warning: {LIB_PATH} is {version!r}, the tree is src={want}", file=sys.stderr)
    elif not version.endswith(f"src={want}"):
        raise RuntimeError(f"{LIB_PATH} ({version!r}) was not built from this tree's sources (src={want}): "
                           f"rebuild it with `make -C {CSRC}`")
    _lib = L
    return L


def synth():
    global _synth
    if _synth is None:
        if not os.path.exists(SYNTH_PATH):
            raise RuntimeError(f"{SYNTH_PATH} is missing: build it with `make -C {CSRC}`")
        S = C.CDLL(SYNTH_PATH)
        S.ngs_synth_corpus.restype = C.c_int
        S.ngs_synth_corpus.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_char_p)),
                                       C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint64)]
        S.ngs_synth_queries.restype = C.c_int
        S.ngs_synth_queries.argtypes = [C.POINTER(C.c_char_p), C.c_uint64, C.c_uint32, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_void_p),
                                        C.POINTER(C.POINTER(C.c_uint64))]
        S.ngs_synth_free.restype = None
        S.ngs_synth_free.argtypes = [C.c_void_p]
        S.ngs_synth_widen.restype = C.c_int
        S.ngs_synth_widen.argtypes = [C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(C.POINTER(C.c_uint32)),
                                      C.POINTER(C.POINTER(C.POINTER(C.c_uint32)))]
        _synth = S
    return _synth


def declared_symbols() -> list[str]:
    """Every function include/ngram_search.h declares with NGS_API."""
    text = open(HEADER).read()
    return re.findall(r"NGS_API\s+[\w\s\*]+?\b(\w+)\s*\(", text)
