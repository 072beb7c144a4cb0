"""Host-side mirror of the reference's interface (StringSearch::StringIndex + dllmain exports).

``StringIndex`` wraps one handle of libngram_search.so the way a host app drives the
reference DLL: ``indexN`` on construction (nGramSearch/dllmain.cpp:37), ``search`` /
``score`` (:61 / :82) returning master keys sorted by score, ``size`` / ``lib_size``
(:120 / :133), ``set_valid_char`` (:142) and ``dispose`` (:110). ``score_batch`` is the
batched extension that puts a whole query batch through one GPU pass.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _native

INT32_MAX = 2**31 - 1


def _b(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("latin-1")


# ngsLastError's codes that are not HIP errors (include/ngram_search.h)
NGS_ERR_INTERNAL = 0x10001
NGS_ERR_QUERY_BUFFER = 0x10002
NGS_ERR_RERANK_LIMIT = 0x10003


# the similarity's metrics (NGS_SIM_* of include/ngram_search.h) and "no term was compared"
METRICS = {"levenshtein": 0, "osa": 1, "partial": 2}
TOKEN_SORT = 0x100  # NGS_SIM_TOKEN_SORT: OR'ed onto a metric
NO_TERM = 0xFFFFFFFF
NO_MATCH = 0xFFFFFFFF  # NGS_NO_MATCH: link() found no key for this one


def _metric(metric, token_sort: bool = False) -> int:
    """"levenshtein" | "osa" | "partial" or the integer (with or without TOKEN_SORT) -> NGS_SIM_*,
    with TOKEN_SORT set if token_sort."""
    flag = TOKEN_SORT if token_sort else 0
    if isinstance(metric, str):
        if metric not in METRICS:
            raise ValueError(f"unknown metric {metric!r}: one of {sorted(METRICS)}")
        return METRICS[metric] | flag
    m = int(metric)
    if (m & ~TOKEN_SORT) not in METRICS.values():
        raise ValueError(f"unknown metric {metric!r}: one of {sorted(METRICS.values())}, with or without "
                         f"TOKEN_SORT ({TOKEN_SORT:#x})")
    return m | flag


def _check(what: str) -> None:
    """Raise if the last call on this thread failed (ngsLastError): the reference's entry points
    answer 0 on failure, which would otherwise read as "no results"."""
    e = _native.lib().ngsLastError(1)
    if e == NGS_ERR_INTERNAL:
        raise RuntimeError(f"{what} failed: a kernel reported an internal error (see stderr)")
    if e == NGS_ERR_QUERY_BUFFER:
        raise RuntimeError(f"{what} failed: the batch outgrew the normalised-query buffer")
    if e == NGS_ERR_RERANK_LIMIT:
        raise ValueError(f"{what} failed: the effective limit (min(limit, keys)) is above 4,096, the most the "
                         f"re-rank takes per query")
    if e:
        raise RuntimeError(f"{what} failed: HIP error {e} (see stderr)")


def _ok(rc: int, what: str, exc=RuntimeError) -> None:
    """Raise if a call that answers a return code answered a non-zero one."""
    if rc:
        raise exc(f"{what} failed: {rc}")


def _cut(counts, nq: int, total: int, *columns):
    """Flat result arrays -> one list per query: query i takes the next counts[i] places of every
    column. A column is an indexable or (indexable, convert). One column gives lists of values, several
    lists of tuples. The counts must add up to `total`."""
    cols = [c if isinstance(c, tuple) else (c, None) for c in columns]
    out, o = [], 0
    for i in range(nq):
        c = counts[i]
        rows = [[f(a[j]) if f else a[j] for j in range(o, o + c)] for a, f in cols]
        out.append(rows[0] if len(rows) == 1 else list(zip(*rows)))
        o += c
    assert o == total
    return out


class StringIndex:
    """One index of byte strings. gram_size 3 is the reference (indexN); 1 or 2 use the indexG
    extension (every reference threshold scaled by the gram size)."""

    def __init__(self, words, row_size: int = 1, weights=None, device: int | None = None, gram_size: int = 3,
                 devices=None):
        """devices: a list of HIP devices to place one replica of the index on each (ngsSetDevices;
        repeats allowed); batches are then split across the replicas."""
        L = _native.lib()
        if devices is not None:
            ds = (C.c_int * max(1, len(devices)))(*devices)
            rc = L.ngsSetDevices(ds, len(devices))
            if rc:
                raise RuntimeError(f"ngsSetDevices({list(devices)}) failed: {rc}")
        elif device is not None:
            rc = L.ngsSetDevice(device)
            if rc:
                raise RuntimeError(f"ngsSetDevice({device}) failed: {rc}")
        n = len(words)
        w = None
        if weights is not None:
            w = (C.c_float * max(1, len(weights)))(*weights)
        self.handle = 0
        try:
            self._keep = self._words(words)  # alive during the build only
            self.handle = self._index(L, self._keep if n else None, n, row_size, w, gram_size)
        finally:
            self._keep = None
            if devices is not None:  # the device list applies to this build only
                L.ngsSetDevices(None, 0)
        if not self.handle:
            raise RuntimeError(f"{self._INDEX} failed (no usable GPU, or gram_size not in 1..3?) — see stderr")

    def save(self, path) -> None:
        """Writes the index to `path` (ngsSaveIndex): the interned library; `load` rebuilds the
        rest on the GPU."""
        _ok(_native.lib().ngsSaveIndex(self.handle, os.fsencode(path)), f"ngsSaveIndex({path!r})", OSError)

    @classmethod
    def load(cls, path, devices=None):
        """An index from a file `save` wrote (ngsLoadIndex), of the same width as the saved one."""
        L = _native.lib()
        if devices is not None:
            ds = (C.c_int * max(1, len(devices)))(*devices)
            _ok(L.ngsSetDevices(ds, len(devices)), f"ngsSetDevices({list(devices)})")
        try:
            handle = L.ngsLoadIndex(os.fsencode(path))
        finally:
            if devices is not None:
                L.ngsSetDevices(None, 0)
        if not handle:
            raise OSError(f"ngsLoadIndex({path!r}) failed: not an index file, or no usable GPU")
        cs = L.ngsCharSize(handle)
        if cs != cls._CS:
            L.dispose(handle)
            raise TypeError(f"{path!r} holds an index of {cs}-byte characters, not {cls.__name__}'s")
        self = cls.__new__(cls)
        self.handle = handle
        self._keep = None
        return self

    # -- per-width plumbing (overridden by WideStringIndex) ------------------------------
    _INDEX = "indexN"
    _CS = 1  # bytes per character

    @staticmethod
    def _words(words):
        arr = (C.c_char_p * max(1, len(words)))()
        for i, w in enumerate(words):
            arr[i] = None if w is None else _b(w)
        return arr

    @staticmethod
    def _index(L, arr, n, row_size, w, gram_size):
        if gram_size == 3:
            return L.indexN(arr, n, row_size, w)
        return L.indexG(arr, n, row_size, w, gram_size)

    _q = staticmethod(_b)
    _string = staticmethod(C.string_at)
    _RES = C.POINTER(C.POINTER(C.c_char))
    _fn = {"search": "search", "score": "score", "release": "release", "scoreBatch": "scoreBatch", "key": "ngsKey",
           "scoreBatchSim": "scoreBatchSim", "scoreBatchSimM": "scoreBatchSimM"}

    def _queries(self, queries):
        return (C.c_char_p * max(1, len(queries)))(*[_b(q) for q in queries])

    # -- reference exports -------------------------------------------------------------
    def size(self) -> int:
        return _native.lib().getSize(self.handle)

    def lib_size(self) -> int:
        return _native.lib().getLibSize(self.handle)

    def set_valid_char(self, chars) -> None:
        b = _b(chars)
        _native.lib().setValidChar(self.handle, b, len(b))

    def score(self, query, threshold: float = 0.0, limit: int = 100):
        """dllmain.cpp:82: list of (key bytes, fp32 score), best first."""
        L, f = _native.lib(), self._fn
        res = self._RES()
        sc = C.POINTER(C.c_float)()
        L.ngsLastError(1)
        n = getattr(L, f["score"])(self.handle, self._q(query), C.byref(res), C.byref(sc), threshold, limit)
        if not n:
            _check(f["score"])
            if res:
                getattr(L, f["release"])(self.handle, res, sc)
            return []
        out = [(self._string(res[i]), sc[i]) for i in range(n)]
        getattr(L, f["release"])(self.handle, res, sc)
        return out

    def search(self, query, threshold: float = 0.0, limit: int = 100):
        """dllmain.cpp:61: list of key bytes, best first."""
        L, f = _native.lib(), self._fn
        res = self._RES()
        L.ngsLastError(1)
        n = getattr(L, f["search"])(self.handle, self._q(query), C.byref(res), threshold, limit)
        if not n:
            _check(f["search"])
        out = [self._string(res[i]) for i in range(n)]
        if res:
            getattr(L, f["release"])(self.handle, res, None)
        return out

    def score_batch(self, queries, threshold: float = 0.0, limit: int = 100):
        """scoreBatch: one list of (key, score) per query."""
        L, f = _native.lib(), self._fn
        nq = len(queries)
        qs = self._queries(queries)
        counts = (C.c_uint32 * max(1, nq))()
        res = self._RES()
        sc = C.POINTER(C.c_float)()
        L.ngsLastError(1)
        total = getattr(L, f["scoreBatch"])(self.handle, qs, nq, threshold, limit, counts, C.byref(res),
                                            C.byref(sc))
        if not total:
            _check(f["scoreBatch"])
        out, o = [], 0
        for i in range(nq):
            c = counts[i]
            out.append([(self._string(res[o + j]), sc[o + j]) for j in range(c)])
            o += c
        assert o == total
        if res:
            getattr(L, f["release"])(self.handle, res, sc)
        return out

    def score_batch_sim(self, queries, threshold: float = 0.0, limit: int = 100, min_similarity: float = 0.0,
                        metric=None, with_terms: bool = False, token_sort: bool = False):
        """scoreBatchSim: score_batch re-ranked by the edit-distance similarity (include/ngram_search.h):
        one list of (key, score, sim) per query, records with sim < min_similarity dropped, the rest in
        order of (sim descending, the search's order ascending). min(limit, keys) must be at most 4,096.
        metric: "levenshtein" (the default), "osa" or "partial", or NGS_SIM_*'s integer (scoreBatchSimM).
        with_terms: every result is (key, score, sim, term), term the matched term's string as `term`
        returns it, None where no term was compared.
        token_sort: the similarity of the token-sorted query and terms (NGS_SIM_TOKEN_SORT): the order of
        the words does not count."""
        by_metric = metric is not None or with_terms or token_sort
        m = _metric("levenshtein" if metric is None else metric, token_sort)
        L = _native.lib()
        fn = self._fn["scoreBatchSimM" if by_metric else "scoreBatchSim"]
        nq = len(queries)
        qs = self._queries(queries)
        counts = (C.c_uint32 * max(1, nq))()
        res = self._RES()
        sc = C.POINTER(C.c_float)()
        sv = C.POINTER(C.c_float)()
        tv = C.POINTER(C.c_uint32)()
        out_args = (counts, C.byref(res), C.byref(sc), C.byref(sv))
        L.ngsLastError(1)
        if by_metric:
            total = getattr(L, fn)(self.handle, qs, nq, threshold, limit, m, min_similarity, *out_args,
                                   C.byref(tv) if with_terms else None)
        else:
            total = getattr(L, fn)(self.handle, qs, nq, threshold, limit, min_similarity, *out_args)
        if not total:
            _check(fn)
        names: dict = {}  # term id -> string: one ngsTerm call per distinct term

        def name(t):
            if t == NO_TERM:
                return None
            if t not in names:
                names[t] = self.term(t)
            return names[t]

        out = _cut(counts, nq, total, (res, self._string), sc, sv, *([(tv, name)] if with_terms else []))
        release = getattr(L, self._fn["release"])
        if res:
            release(self.handle, res, sc)
        if sv:
            release(self.handle, None, sv)
        if tv:
            L.ngsReleaseTerms(tv)
        return out

    def term(self, term_id: int):
        """ngsTerm: the normalised term `term_id` (0 .. size() - 1) as the index holds it, in the type
        this class returns keys in. One small device copy per call: for showing results, not for export."""
        L = _native.lib()
        n = L.ngsTerm(self.handle, term_id, None, 0)
        if n < 0:
            raise IndexError(term_id) if n == -3 else RuntimeError(f"ngsTerm failed: {n}")
        buf = (C.c_uint8 * max(1, n * self._CS))()
        got = L.ngsTerm(self.handle, term_id, buf, n * self._CS)
        if got != n:
            raise RuntimeError(f"ngsTerm failed: {got}")
        return self._term_string(bytes(buf[:n * self._CS]))

    _term_string = staticmethod(bytes)

    def dispose(self) -> None:
        if self.handle:
            _native.lib().dispose(self.handle)
            self.handle = 0

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    # -- device-level extension ---------------------------------------------------------
    def num_keys(self) -> int:
        return _native.lib().ngsNumKeys(self.handle)

    def key(self, key_id: int):
        p = getattr(_native.lib(), self._fn["key"])(self.handle, key_id)
        if not p:
            raise IndexError(key_id)
        return self._string(p)

    def replicas(self) -> int:
        """Devices the index was placed on (ngsReplicaCount)."""
        return _native.lib().ngsReplicaCount(self.handle)

    def gram_size(self) -> int:
        return _native.lib().ngsGramSize(self.handle)

    def serve(self, enable: bool = True) -> None:
        """ngsServe: single score()/search() calls through the persistent low-latency server (on a
        small library it also starts by itself after the 4th call; serve(False) turns that off)."""
        rc = _native.lib().ngsServe(self.handle, int(enable))
        if rc:
            raise RuntimeError(f"ngsServe failed: {rc}")

    def serve_state(self) -> int:
        """ngsServeState: 0 no server, 1 set up but its kernel stopped, 2 its kernel running."""
        return _native.lib().ngsServeState(self.handle)

    def set_timing(self, enable: bool = True) -> None:
        _native.lib().ngsSetTiming(self.handle, int(enable))

    def last_stats(self) -> dict:
        st = _native.NgsStats()
        _native.lib().ngsLastStats(self.handle, C.byref(st))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def key_lengths_device(self, first: int, count: int, d_len: int, stream: int = 0) -> None:
        """ngsKeyLengthsDevice: d_len[i] = the characters of key first + i, queued on `stream`."""
        _ok(_native.lib().ngsKeyLengthsDevice(self.handle, first, count, d_len or None, stream or None),
            "ngsKeyLengthsDevice")

    def search_device(self, d_bytes: int, d_offsets: int, n: int, threshold: float, limit: int, out_stride: int,
                      d_counts: int, d_keys: int, d_scores: int, stream: int = 0) -> None:
        """ngsSearchDevice on raw device pointers (e.g. torch tensors' data_ptr())."""
        _ok(_native.lib().ngsSearchDevice(self.handle, d_bytes, d_offsets, n, threshold, limit, out_stride,
                                          d_counts, d_keys, d_scores, stream or None), "ngsSearchDevice")

    def similarity_device(self, d_bytes: int, d_offsets: int, n: int, stride: int, d_counts: int, d_keys: int,
                          d_sim: int, stream: int = 0, metric=None, d_terms: int = 0, token_sort: bool = False) -> None:
        """ngsSimilarityDevice on raw device pointers: d_sim[i * stride + r] = the edit-distance similarity of
        query i and key d_keys[i * stride + r], r < d_counts[i]; queued on `stream`, nothing waits.
        With a metric or d_terms (the matched term ids, in d_sim's layout): ngsSimilarityDeviceM.
        token_sort sets NGS_SIM_TOKEN_SORT only: the token-sorted terms are read and the query bytes taken
        as given (token_sort_device on the same stream first)."""
        L, head = _native.lib(), (self.handle, d_bytes, d_offsets, n, stride, d_counts, d_keys)
        if metric is not None or d_terms or token_sort:
            _ok(L.ngsSimilarityDeviceM(*head, _metric("levenshtein" if metric is None else metric, token_sort), d_sim,
                                       d_terms or None, stream or None), "ngsSimilarityDeviceM")
        else:
            _ok(L.ngsSimilarityDevice(*head, d_sim, stream or None), "ngsSimilarityDevice")

    def token_sort_device(self, d_bytes: int, d_offsets: int, n: int, d_out: int, stream: int = 0) -> None:
        """ngsTokenSortDevice on raw device pointers: the n strings of a query batch token-sorted into d_out
        at the same offsets (d_out may be d_bytes), under this index's width and validChar set; queued
        on `stream`."""
        _ok(_native.lib().ngsTokenSortDevice(self.handle, d_bytes or None, d_offsets or None, n, d_out or None,
                                             stream or None), "ngsTokenSortDevice")

    def rerank_device(self, d_bytes: int, d_offsets: int, n: int, stride: int, d_counts: int, d_keys: int,
                      d_scores: int, d_sim: int, min_similarity: float = 0.0, stream: int = 0, metric=None,
                      d_terms: int = 0, token_sort: bool = False) -> None:
        """ngsRerankDevice on raw device pointers: the similarity, then every query's records filtered by
        min_similarity and ordered by (sim descending, position ascending), in place; queued on `stream`.
        With a metric or d_terms (the matched term ids, permuted with the records): ngsRerankDeviceM.
        token_sort: as similarity_device's."""
        L, head = _native.lib(), (self.handle, d_bytes, d_offsets, n, stride, d_counts, d_keys, d_scores, d_sim)
        if metric is not None or d_terms or token_sort:
            _ok(L.ngsRerankDeviceM(*head, d_terms or None,
                                   _metric("levenshtein" if metric is None else metric, token_sort),
                                   min_similarity, stream or None), "ngsRerankDeviceM")
        else:
            _ok(L.ngsRerankDevice(*head, min_similarity, stream or None), "ngsRerankDevice")

    # -- self-join: near-duplicate keys and their clusters (include/ngram_search.h) ----------
    def self_join(self, first: int = 0, count: int | None = None, threshold: float = 0.0, limit: int = 10):
        """selfJoin: for each key first .. first + count - 1 (default: to the last key) the list of
        (key_id, score) the search gives for the key's own string, over the library without that key."""
        L = _native.lib()
        nk = self.num_keys()
        n = max(0, nk - first) if count is None else count
        stride = max(1, min(limit if limit else INT32_MAX, nk))
        counts = (C.c_uint32 * max(1, n))()
        keys = (C.c_uint32 * max(1, n * stride))()
        scores = (C.c_float * max(1, n * stride))()
        L.ngsLastError(1)
        total = L.selfJoin(self.handle, first, n, threshold, limit, stride, counts, keys, scores)
        if not total:
            _check("selfJoin")
        out = [list(zip(keys[i * stride:i * stride + counts[i]], scores[i * stride:i * stride + counts[i]]))
               for i in range(n)]
        assert sum(map(len, out)) == total
        return out

    def dedup(self, threshold: float, limit: int = 10, min_similarity: float | None = None, batch_keys: int = 0,
              metric=None, token_sort: bool = False):
        """dedupKeys: labels[k] = the smallest key id of key k's cluster, the clusters being the
        connected components of the self-join at (threshold, limit); with min_similarity, of its records
        whose edit-distance similarity is at least that. limit in 1..4,096. metric: the similarity's
        (dedupKeysM); "partial" is directional, and an edge is made if either key's row keeps it.
        token_sort: the similarity of the token-sorted strings, so keys whose words are in another order
        join."""
        if token_sort and metric is None:
            metric = "levenshtein"
        L = _native.lib()
        nk = self.num_keys()
        labels = (C.c_uint32 * max(1, nk))()
        L.ngsLastError(1)
        ms = -1.0 if min_similarity is None else min_similarity
        if metric is None:
            clusters = L.dedupKeys(self.handle, threshold, limit, ms, batch_keys, labels)
        else:
            clusters = L.dedupKeysM(self.handle, threshold, limit, _metric(metric, token_sort), ms, batch_keys,
                                    labels)
        if not clusters:
            _check("dedupKeys" if metric is None else "dedupKeysM")
        out = list(labels[:nk])
        assert clusters == sum(1 for k, v in enumerate(out) if k == v)
        return out

    def key_query_bytes(self, first: int, count: int) -> int:
        """ngsKeyQueryBytes: the bytes keys first .. first + count - 1 take as a query batch."""
        return _native.lib().ngsKeyQueryBytes(self.handle, first, count)

    def key_queries_device(self, first: int, count: int, d_bytes: int, cap_bytes: int, d_offsets: int,
                           stream: int = 0) -> None:
        """ngsKeyQueriesDevice on raw device pointers: those keys in search_device's query layout, queued
        on `stream`."""
        _ok(_native.lib().ngsKeyQueriesDevice(self.handle, first, count, d_bytes or None, cap_bytes, d_offsets,
                                              stream or None), "ngsKeyQueriesDevice")

    @staticmethod
    def drop_self_device(d_counts: int, d_keys: int, d_scores: int, n: int, stride: int, first: int, limit: int = 0,
                         stream: int = 0) -> None:
        """ngsDropSelfDevice on raw device pointers: row i loses the record of key first + i and is cut to
        `limit` (0: no cut), in place; queued on `stream`."""
        _ok(_native.lib().ngsDropSelfDevice(d_counts, d_keys or None, d_scores or None, n, stride, first, limit,
                                            stream or None), "ngsDropSelfDevice")

    def self_join_device(self, first: int, count: int, threshold: float, limit: int, out_stride: int, d_counts: int,
                         d_keys: int, d_scores: int, stream: int = 0) -> None:
        """ngsSelfJoinDevice on raw device pointers; out_stride >= min((limit or 2^31-1) + 1, keys)."""
        _ok(_native.lib().ngsSelfJoinDevice(self.handle, first, count, threshold, limit, out_stride, d_counts,
                                            d_keys or None, d_scores or None, stream or None), "ngsSelfJoinDevice")

    @staticmethod
    def cluster_device(d_counts: int, d_keys: int, n: int, stride: int, first: int, d_labels: int, n_labels: int,
                       init: bool = True, finish: bool = True, stream: int = 0) -> None:
        """ngsClusterDevice on raw device pointers: the block's (first + i, key) records merged into the
        label forest d_labels[n_labels]; `init` sets labels[k] = k first, `finish` makes every label the
        smallest id of its component. Queued on `stream`."""
        _ok(_native.lib().ngsClusterDevice(d_counts or None, d_keys or None, n, stride, first, d_labels or None,
                                           n_labels, (1 if init else 0) | (2 if finish else 0), stream or None),
            "ngsClusterDevice")

    # -- linking two indexes (include/ngram_search.h) -----------------------------------------
    def link(self, other, threshold: float, limit: int = 10, min_similarity: float | None = None,
             metric="levenshtein", token_sort: bool = False, one_to_one: bool = True, batch_keys: int = 0):
        """linkKeys: every key of this index searched in `other` (same character width) at (threshold,
        limit), limit in 1..4,096. Returns numpy arrays (match, scores, sims) over this index's keys:
        match[a] = the key id of `other` linked to key a, or NO_MATCH; scores[a] and sims[a] those of
        the chosen record (0.0 and -1.0 for an unmatched key). With min_similarity only the records
        whose similarity by `metric` (token_sort: of the token-sorted strings) is at least that count,
        and they are ranked by it; without it they are ranked by score and sims is None.
        one_to_one: the greedy matching (the best record overall first; no key of `other` is given
        twice); otherwise every key takes its best record."""
        import numpy as np
        L = _native.lib()
        if L.ngsCharSize(self.handle) != L.ngsCharSize(other.handle):
            raise ValueError("link: the two indexes differ in character width")
        n = self.num_keys()
        match = np.full(max(1, n), NO_MATCH, dtype=np.uint32)
        scores = np.zeros(max(1, n), dtype=np.float32)
        sims = np.full(max(1, n), -1.0, dtype=np.float32)
        ms = -1.0 if min_similarity is None else min_similarity
        L.ngsLastError(1)
        matched = L.linkKeys(self.handle, other.handle, threshold, limit, _metric(metric, token_sort), ms,
                             1 if one_to_one else 0, batch_keys, match.ctypes.data_as(C.POINTER(C.c_uint32)),
                             scores.ctypes.data_as(C.POINTER(C.c_float)), sims.ctypes.data_as(C.POINTER(C.c_float)))
        if not matched:
            _check("linkKeys")
        match, scores, sims = match[:n], scores[:n], sims[:n]
        assert matched == int((match != NO_MATCH).sum())
        return match, scores, (sims if min_similarity is not None and ms > -1.0 else None)

    @staticmethod
    def match_device(d_counts: int, d_keys: int, d_values: int, n: int, stride: int, first: int, d_match_a: int,
                     n_a: int, d_match_b: int, n_b: int, d_bids: int, d_matched: int, init: bool = False,
                     begin: bool = True, bid: bool = True, accept: bool = True, stream: int = 0) -> None:
        """ngsMatchDevice on raw device pointers: one step of the greedy one-to-one matching over the block's
        (first + i, key, value) records. `init` frees every end and zeroes the pair count, `begin` starts a
        round (the bids cleared), `bid` lets the block's live records bid, `accept` takes the records that
        won at both ends and adds them to the count at d_matched. A round over one block is the default
        flags; repeat until the count stops growing. Queued on `stream`."""
        flags = (1 if init else 0) | (2 if begin else 0) | (4 if bid else 0) | (8 if accept else 0)
        _ok(_native.lib().ngsMatchDevice(d_counts or None, d_keys or None, d_values or None, n, stride, first,
                                         d_match_a or None, n_a, d_match_b or None, n_b, d_bids or None,
                                         d_matched or None, flags, stream or None), "ngsMatchDevice")

    def search_device_async(self, d_bytes: int, d_offsets: int, n: int, threshold: float, limit: int,
                            out_stride: int, d_counts: int, d_keys: int, d_scores: int, stream: int = 0) -> int:
        """ngsSearchDeviceAsync: queues the search and returns its ticket (wait_device(ticket))."""
        t = C.c_uint64()
        _ok(_native.lib().ngsSearchDeviceAsync(self.handle, d_bytes, d_offsets, n, threshold, limit, out_stride,
                                               d_counts, d_keys, d_scores, stream or None, C.byref(t)),
            "ngsSearchDeviceAsync")
        return t.value

    def wait_device(self, ticket: int) -> None:
        """ngsSearchDeviceWait: the results of that call are complete on return."""
        _ok(_native.lib().ngsSearchDeviceWait(self.handle, ticket), "ngsSearchDeviceWait")


# ---- wide strings (indexW extension) ---------------------------------------------------
_U32P = C.POINTER(C.c_uint32)


def _u32(s):
    """str (one unit per code point) or a sequence of ints -> NUL-terminated uint32 array."""
    units = [ord(c) for c in s] if isinstance(s, str) else [int(c) & 0xFFFFFFFF for c in s]
    return (C.c_uint32 * (len(units) + 1))(*units, 0)


def _wstring(p) -> str:
    """NUL-terminated UTF-32 string at p -> str (raises on units above 0x10FFFF)."""
    u = C.cast(p, _U32P)
    out = []
    i = 0
    while u[i]:
        out.append(chr(u[i]))
        i += 1
    return "".join(out)


class WideStringIndex(StringIndex):
    """indexW / searchW / scoreW (Readme.md:91,135): UTF-32 strings (Python str, or sequences
    of ints for raw code units such as values above 0x10FFFF), gram_size 1..3."""

    _INDEX = "indexW"
    _CS = 4
    _RES = C.POINTER(_U32P)
    _fn = {"search": "searchW", "score": "scoreW", "release": "releaseW", "scoreBatch": "scoreBatchW",
           "key": "ngsKeyW", "scoreBatchSim": "scoreBatchSimW", "scoreBatchSimM": "scoreBatchSimMW"}

    def __init__(self, words, row_size: int = 1, weights=None, device: int | None = None, gram_size: int = 2,
                 devices=None):
        super().__init__(words, row_size, weights, device, gram_size, devices)

    @staticmethod
    def _words(words):
        arrs = [None if w is None else _u32(w) for w in words]
        arr = (_U32P * max(1, len(words)))(*[None if a is None else C.cast(a, _U32P) for a in arrs])
        arr._arrs = arrs  # keep the strings alive with the pointer array
        return arr

    @staticmethod
    def _index(L, arr, n, row_size, w, gram_size):
        return L.indexW(arr, n, row_size, w, gram_size)

    @staticmethod
    def _q(query):
        return C.cast(_u32(query), _U32P)

    _string = staticmethod(_wstring)
    _term_string = staticmethod(lambda b: "".join(map(chr, memoryview(b).cast("I"))))

    def _queries(self, queries):
        arrs = [_u32(q) for q in queries]
        arr = (_U32P * max(1, len(queries)))(*[C.cast(a, _U32P) for a in arrs])
        arr._arrs = arrs
        return arr

    def size(self) -> int:
        return _native.lib().getSizeW(self.handle)

    def lib_size(self) -> int:
        return _native.lib().getLibSizeW(self.handle)

    def dispose(self) -> None:
        if self.handle:
            _native.lib().disposeW(self.handle)
            self.handle = 0


# ---- UTF-8 strings on a wide index (indexU8 extension) ----------------------------------
def _u8(s) -> bytes:
    """str -> UTF-8 (lone surrogates U+DC80..DCFF back to the bytes they stand for); bytes as they are."""
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8", "surrogateescape")


def _u8string(p) -> str:
    return C.string_at(p).decode("utf-8", "surrogateescape")


def utf8_decode_device(d_bytes: int, d_offsets: int, n: int, d_out: int, out_cap_bytes: int, d_out_offsets: int,
                       stream: int = 0) -> None:
    """ngsUtf8Decode on raw device pointers: n UTF-8 strings (absolute byte offsets) -> UTF-32
    characters in d_out and their byte offsets (from 0) in d_out_offsets, queued on `stream`."""
    _ok(_native.lib().ngsUtf8Decode(d_bytes, d_offsets, n, d_out, out_cap_bytes, d_out_offsets, stream or None),
        "ngsUtf8Decode")


class Utf8StringIndex(WideStringIndex):
    """indexU8 / searchU8 / scoreU8 / scoreBatchU8: a wide index driven with UTF-8. Words and
    queries are str (encoded with 'utf-8', 'surrogateescape') or bytes (taken as they are);
    results are str decoded the same way, so bytes that are not UTF-8 come back as U+DC80..DCFF."""

    _INDEX = "indexU8"
    _RES = C.POINTER(C.POINTER(C.c_char))
    _fn = {"search": "searchU8", "score": "scoreU8", "release": "release", "scoreBatch": "scoreBatchU8",
           "key": "ngsKeyU8", "scoreBatchSim": "scoreBatchSimU8", "scoreBatchSimM": "scoreBatchSimMU8"}

    @staticmethod
    def _words(words):
        arr = (C.c_char_p * max(1, len(words)))()
        for i, w in enumerate(words):
            arr[i] = None if w is None else _u8(w)
        return arr

    @staticmethod
    def _index(L, arr, n, row_size, w, gram_size):
        return L.indexU8(arr, n, row_size, w, gram_size)

    _q = staticmethod(_u8)
    _string = staticmethod(_u8string)

    def _queries(self, queries):
        return (C.c_char_p * max(1, len(queries)))(*[_u8(q) for q in queries])

    def search_device_u8(self, d_bytes: int, d_offsets: int, n: int, threshold: float, limit: int, out_stride: int,
                         d_counts: int, d_keys: int, d_scores: int, stream: int = 0) -> None:
        """ngsSearchDeviceU8: search_device with UTF-8 query bytes and offsets."""
        _ok(_native.lib().ngsSearchDeviceU8(self.handle, d_bytes, d_offsets, n, threshold, limit, out_stride,
                                            d_counts, d_keys, d_scores, stream or None), "ngsSearchDeviceU8")


# ---- index sets: several indexes searched as one library (include/ngram_search.h) --------
def merge_results_device(parts, n: int, limit: int, out_stride: int, d_counts: int, d_keys: int, d_scores: int,
                         stream: int = 0) -> None:
    """ngsMergeResultsDevice on raw device pointers. parts: up to 16 of (d_counts, d_keys, d_scores, stride,
    key_base, d_key_len, n_keys), each a result block of ngsSearchDevice's layout for the same n queries
    with its keys' lengths (key_lengths_device); the output block is what one index over all the parts'
    rows would have answered, with key ids key_base + k. Queued on `stream`; nothing waits."""
    arr = (_native.MergePart * max(1, len(parts)))()
    for a, (pc, pk, ps, stride, base, plen, nk) in zip(arr, parts):
        a.dCounts, a.dKeys, a.dScores, a.dKeyLen = pc or None, pk or None, ps or None, plen or None
        a.stride, a.keyBase, a.nKeys = stride, base, nk
    _ok(_native.lib().ngsMergeResultsDevice(arr, len(parts), n, limit, out_stride, d_counts, d_keys, d_scores,
                                            stream or None), "ngsMergeResultsDevice")


def drop_dead_device(d_counts: int, d_keys: int, d_scores: int, n: int, stride: int, d_dead: int, n_keys: int,
                     limit: int = 0, d_short: int = 0, stream: int = 0) -> None:
    """ngsDropDeadDevice on raw device pointers: the records of every row of the block whose key k < n_keys
    has bit k & 31 of d_dead[k >> 5] set are removed in place, the rest keep their order and move up, the
    row is cut to `limit`; *d_short (may be 0) is increased by the rows that filled the stride and were
    left with fewer than `limit` records. Queued on `stream`; nothing waits."""
    _ok(_native.lib().ngsDropDeadDevice(d_counts, d_keys or None, d_scores or None, n, stride, d_dead or None, n_keys,
                                        limit, d_short or None, stream or None), "ngsDropDeadDevice")


class IndexSet:
    """Indexes of one class and gram size searched as one library (ngsSet*): partitions of a library, or a
    base and the parts appended to it. Global key id = the keys of the earlier parts + the local id; the
    answers are those of one index over all the parts' rows when no master key is in two parts. The set
    holds its members (none is collected under it) but does not own them: dispose() leaves them alive."""

    def __init__(self, parts):
        parts = list(parts)
        if not parts:
            raise ValueError("an IndexSet needs at least one index")
        L = _native.lib()
        hs = (C.c_uint32 * len(parts))(*[p.handle for p in parts])
        L.ngsLastError(1)
        self.set_id = L.ngsSetCreate(hs, len(parts))
        if not self.set_id:
            raise RuntimeError(f"ngsSetCreate failed: error {L.ngsLastError(1)} (1..16 built indexes of one "
                               f"character and gram size on one device)")
        self._parts = parts

    @property
    def parts(self):
        return list(self._parts)

    def add(self, index) -> None:
        """ngsSetAdd: `index` becomes the last part; the ids of the keys already there stay."""
        _ok(_native.lib().ngsSetAdd(self.set_id, index.handle), "ngsSetAdd")
        self._parts.append(index)

    def append(self, words, row_size: int = 1, weights=None):
        """Builds an index of the first part's class and gram size over `words` and adds it; returns it."""
        first = self._parts[0]
        index = type(first)(words, row_size, weights, gram_size=first.gram_size())
        try:
            self.add(index)
        except Exception:
            index.dispose()
            raise
        return index

    def num_keys(self) -> int:
        return _native.lib().ngsSetNumKeys(self.set_id)

    def locate(self, key_id: int):
        """(member index, local key id) of a global key id."""
        h, k = C.c_uint32(), C.c_uint32()
        if _native.lib().ngsSetLocate(self.set_id, key_id, C.byref(h), C.byref(k)):
            raise IndexError(key_id)
        return next(p for p in self._parts if p.handle == h.value), k.value

    def key(self, key_id: int):
        index, k = self.locate(key_id)
        return index.key(k)

    # -- dead keys: delete without a rebuild; to update a key, remove it and append the new row --
    def _mark(self, what: str, key_ids) -> int:
        ids = [int(g) for g in key_ids]
        arr = (C.c_uint32 * max(1, len(ids)))(*ids)
        rc = getattr(_native.lib(), what)(self.set_id, arr, len(ids))
        if rc == -3:
            raise IndexError(f"{what}: a key id at or past num_keys() (nothing was changed)")
        _ok(min(rc, 0), what)
        return rc

    def remove(self, key_ids) -> int:
        """ngsSetRemove: the global key ids become dead and leave every later answer of the set, which is
        then that of a set without those keys' rows; ids, strings and the members stay as they are.
        Returns the number of keys newly dead; IndexError, with nothing changed, for an id past the set."""
        return self._mark("ngsSetRemove", key_ids)

    def restore(self, key_ids) -> int:
        """ngsSetRestore: the global key ids become live again; returns the number newly live."""
        return self._mark("ngsSetRestore", key_ids)

    def live_keys(self) -> int:
        return _native.lib().ngsSetLiveKeys(self.set_id)

    def dead_keys(self):
        """The dead global key ids, ascending: what a caller stores to persist the set's deletions."""
        L = _native.lib()
        n = L.ngsSetDeadKeys(self.set_id, None, 0)
        out = (C.c_uint32 * max(1, n))()
        n = min(n, L.ngsSetDeadKeys(self.set_id, out, n))
        return list(out[:n])

    def is_live(self, key_id: int) -> bool:
        rc = _native.lib().ngsSetIsLive(self.set_id, key_id)
        if rc == -3:
            raise IndexError(key_id)
        _ok(min(rc, 0), "ngsSetIsLive")
        return bool(rc)

    def dead_stats(self) -> dict:
        """ngsSetDeadStats: counters since the set was made."""
        out = (C.c_uint64 * 3)()
        rc = _native.lib().ngsSetDeadStats(self.set_id, out, 3)
        _ok(min(rc, 0), "ngsSetDeadStats")
        return {"drop_launches": out[0], "re_searches": out[1], "max_over_fetch": out[2]}

    def score_batch(self, queries, threshold: float = 0.0, limit: int = 100):
        """scoreBatchSet / W / U8 by the members' class: one list of (key, score) per query."""
        L, first = _native.lib(), self._parts[0]
        what = "scoreBatchSet" + first._fn["scoreBatch"][len("scoreBatch"):]
        fn = getattr(L, what)
        nq = len(queries)
        qs = first._queries(queries)
        stride = max(1, min(limit if limit else INT32_MAX, self.num_keys()))
        counts = (C.c_uint32 * max(1, nq))()
        keys = (C.c_uint32 * max(1, nq * stride))()
        scores = (C.c_float * max(1, nq * stride))()
        L.ngsLastError(1)
        total = fn(self.set_id, qs, nq, threshold, limit, stride, counts, keys, scores)
        if not total:
            _check(what)
        strings = {}

        def name(g):
            if g not in strings:
                strings[g] = self.key(g)
            return strings[g]

        out = [[(name(keys[i * stride + j]), scores[i * stride + j]) for j in range(counts[i])] for i in range(nq)]
        assert sum(map(len, out)) == total
        return out

    def search_device(self, d_bytes: int, d_offsets: int, n: int, threshold: float, limit: int, out_stride: int,
                      d_counts: int, d_keys: int, d_scores: int, stream: int = 0) -> None:
        """ngsSetSearchDevice on raw device pointers: search_device over the set, keys as global ids."""
        _ok(_native.lib().ngsSetSearchDevice(self.set_id, d_bytes, d_offsets, n, threshold, limit, out_stride,
                                             d_counts, d_keys, d_scores, stream or None), "ngsSetSearchDevice")

    # -- the later stages over the set (include/ngram_search.h): StringIndex's methods, global key ids --
    def _stride(self, limit: int) -> int:
        return max(1, min(limit if limit else INT32_MAX, self.num_keys()))

    def term(self, key_id: int, term_id: int):
        """The matched term `term_id` of a record whose key is the global `key_id`: term ids are local to
        the member that holds the key."""
        index, _ = self.locate(key_id)
        return index.term(term_id)

    def score_batch_sim(self, queries, threshold: float = 0.0, limit: int = 100, min_similarity: float = 0.0,
                        metric=None, with_terms: bool = False, token_sort: bool = False):
        """scoreBatchSetSimM / W / U8: StringIndex.score_batch_sim over the set. One list of (key, score, sim)
        per query, with_terms (key, score, sim, term)."""
        L, first = _native.lib(), self._parts[0]
        what = "scoreBatchSetSimM" + first._fn["scoreBatch"][len("scoreBatch"):]
        m = _metric("levenshtein" if metric is None else metric, token_sort)
        nq = len(queries)
        qs = first._queries(queries)
        stride = self._stride(limit)
        counts = (C.c_uint32 * max(1, nq))()
        keys = (C.c_uint32 * max(1, nq * stride))()
        scores = (C.c_float * max(1, nq * stride))()
        sims = (C.c_float * max(1, nq * stride))()
        terms = (C.c_uint32 * max(1, nq * stride))() if with_terms else None
        L.ngsLastError(1)
        total = getattr(L, what)(self.set_id, qs, nq, threshold, limit, m, min_similarity, stride, counts, keys, scores,
                                 sims, terms)
        if not total:
            _check(what)
        strings, names = {}, {}

        def name(g):
            if g not in strings:
                strings[g] = self.key(g)
            return strings[g]

        def term(g, t):
            if t == NO_TERM:
                return None
            index, _ = self.locate(g)
            if (index.handle, t) not in names:
                names[index.handle, t] = index.term(t)
            return names[index.handle, t]

        out = []
        for i in range(nq):
            at = range(i * stride, i * stride + counts[i])
            out.append([(name(keys[j]), scores[j], sims[j]) + ((term(keys[j], terms[j]),) if with_terms else ())
                        for j in at])
        assert sum(map(len, out)) == total
        return out

    def self_join(self, first: int = 0, count: int | None = None, threshold: float = 0.0, limit: int = 10):
        """selfJoinSet: StringIndex.self_join over the set's global key ids."""
        L = _native.lib()
        n = max(0, self.num_keys() - first) if count is None else count
        stride = self._stride(limit)
        counts = (C.c_uint32 * max(1, n))()
        keys = (C.c_uint32 * max(1, n * stride))()
        scores = (C.c_float * max(1, n * stride))()
        L.ngsLastError(1)
        total = L.selfJoinSet(self.set_id, first, n, threshold, limit, stride, counts, keys, scores)
        if not total:
            _check("selfJoinSet")
        out = [list(zip(keys[i * stride:i * stride + counts[i]], scores[i * stride:i * stride + counts[i]]))
               for i in range(n)]
        assert sum(map(len, out)) == total
        return out

    def dedup(self, threshold: float, limit: int = 10, min_similarity: float | None = None, batch_keys: int = 0,
              metric=None, token_sort: bool = False):
        """dedupKeysSet: StringIndex.dedup over the set; labels[g] = the smallest global key id of key g's
        cluster."""
        L = _native.lib()
        nk = self.num_keys()
        labels = (C.c_uint32 * max(1, nk))()
        L.ngsLastError(1)
        ms = -1.0 if min_similarity is None else min_similarity
        clusters = L.dedupKeysSet(self.set_id, threshold, limit, _metric("levenshtein" if metric is None else metric,
                                                                          token_sort), ms, batch_keys, labels)
        if not clusters:
            _check("dedupKeysSet")
        out = list(labels[:nk])
        # (a dead key is alone under its own label and is not counted)
        assert clusters == sum(1 for k, v in enumerate(out) if k == v) - (nk - self.live_keys())
        return out

    def similarity_device(self, d_bytes: int, d_offsets: int, n: int, stride: int, d_counts: int, d_keys: int,
                          d_sim: int, stream: int = 0, metric=None, d_terms: int = 0, token_sort: bool = False) -> None:
        """ngsSetSimilarityDeviceM on raw device pointers: StringIndex.similarity_device with global key ids;
        d_terms receives the members' local term ids."""
        _ok(_native.lib().ngsSetSimilarityDeviceM(
            self.set_id, d_bytes, d_offsets, n, stride, d_counts, d_keys,
            _metric("levenshtein" if metric is None else metric, token_sort), d_sim, d_terms or None, stream or None),
            "ngsSetSimilarityDeviceM")

    def rerank_device(self, d_bytes: int, d_offsets: int, n: int, stride: int, d_counts: int, d_keys: int,
                      d_scores: int, d_sim: int, min_similarity: float = 0.0, stream: int = 0, metric=None,
                      d_terms: int = 0, token_sort: bool = False) -> None:
        """ngsSetRerankDeviceM on raw device pointers: StringIndex.rerank_device with global key ids."""
        _ok(_native.lib().ngsSetRerankDeviceM(
            self.set_id, d_bytes, d_offsets, n, stride, d_counts, d_keys, d_scores, d_sim, d_terms or None,
            _metric("levenshtein" if metric is None else metric, token_sort), min_similarity, stream or None),
            "ngsSetRerankDeviceM")

    def key_query_bytes(self, first: int, count: int) -> int:
        """ngsSetKeyQueryBytes: the bytes the global keys first .. first + count - 1 take as a query batch."""
        return _native.lib().ngsSetKeyQueryBytes(self.set_id, first, count)

    def key_queries_device(self, first: int, count: int, d_bytes: int, cap_bytes: int, d_offsets: int,
                           stream: int = 0) -> None:
        """ngsSetKeyQueriesDevice on raw device pointers: those keys in search_device's query layout."""
        _ok(_native.lib().ngsSetKeyQueriesDevice(self.set_id, first, count, d_bytes or None, cap_bytes, d_offsets,
                                                 stream or None), "ngsSetKeyQueriesDevice")

    def self_join_device(self, first: int, count: int, threshold: float, limit: int, out_stride: int, d_counts: int,
                         d_keys: int, d_scores: int, stream: int = 0) -> None:
        """ngsSetSelfJoinDevice on raw device pointers; out_stride >= min((limit or 2^31-1) + 1, keys)."""
        _ok(_native.lib().ngsSetSelfJoinDevice(self.set_id, first, count, threshold, limit, out_stride, d_counts,
                                               d_keys or None, d_scores or None, stream or None),
            "ngsSetSelfJoinDevice")

    def dispose(self) -> None:
        """Disposes the set; the members stay."""
        if self.set_id:
            _native.lib().ngsSetDispose(self.set_id)
            self.set_id = 0

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass
