"""The return codes of the device entry points, and which code wins where two conditions are broken
at once: a table over ngsSearchDevice, ngsSearchDeviceU8, ngsSearchDeviceAsync, ngsSimilarityDevice(M),
ngsRerankDevice(M), ngsKeyQueriesDevice, ngsSelfJoinDevice and ngsTerm on a 50-key narrow library, a
50-key wide one, a handle whose library was never built (one word) and a handle that does not exist.

Every call here is refused by its argument checks. The pointers are those of one live device buffer;
no refused call reads or writes it (ngsTerm's last case copies the term's span first, from the index).
"""
import ctypes as C

import pytest

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAN = float("nan")
UNKNOWN = 0x7FFFFFF0  # no handle has this number


@pytest.fixture(scope="module")
def env():
    words = [b"KEY NUMBER %02d %s" % (i, bytes([65 + i % 26]) * (3 + i % 5)) for i in range(50)]
    narrow = ssl.StringIndex(words, 1)
    wide = ssl.WideStringIndex([w.decode() for w in words], 1, gram_size=2)
    L = _native.lib()
    one = (C.c_char_p * 1)(b"ONLY")
    unbuilt = L.indexN(one, 1, 1, None)
    assert narrow.num_keys() == 50 and wide.num_keys() == 50 and unbuilt
    buf = torch.zeros(1 << 16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    yield {"N": narrow.handle, "W": wide.handle, "E": unbuilt, "X": UNKNOWN, "p": buf.data_ptr(), "ix": narrow,
           "wix": wide}
    narrow.dispose()
    wide.dispose()
    L.dispose(unbuilt)


def _cases(e):
    """(name, function, arguments, expected code): arguments in the export's order, P a good pointer."""
    P = e["p"]
    out = []

    def search(fn, h, off=P, n=4, limit=10, stride=10, cnt=P, keys=P, sc=P, extra=()):
        return (fn, (h, P, off, n, 0.0, limit, stride, cnt, keys, sc, None) + tuple(extra))

    def add(name, call, want):
        out.append((name, call[0], call[1], want))

    # ---- ngsSearchDevice / U8 / Async: handle, then built, (U8: then width), then pointers and stride
    tick = C.c_uint64()
    for fn, h, extra in (("ngsSearchDevice", "N", ()), ("ngsSearchDevice", "W", ()), ("ngsSearchDeviceU8", "W", ()),
                         ("ngsSearchDeviceAsync", "N", (C.byref(tick),))):
        kw = {"extra": extra}
        add(f"{fn}[{h}] unknown handle", search(fn, e["X"], **kw), -1)
        add(f"{fn}[{h}] unknown handle and null offsets", search(fn, e["X"], off=None, **kw), -1)
        add(f"{fn}[{h}] unbuilt handle", search(fn, e["E"], **kw), -2)
        add(f"{fn}[{h}] unbuilt handle and null counts", search(fn, e["E"], cnt=None, **kw), -2)
        add(f"{fn}[{h}] null offsets", search(fn, e[h], off=None, **kw), -3)
        add(f"{fn}[{h}] null counts", search(fn, e[h], cnt=None, **kw), -3)
        add(f"{fn}[{h}] null keys", search(fn, e[h], keys=None, **kw), -3)
        add(f"{fn}[{h}] null scores", search(fn, e[h], sc=None, **kw), -3)
        add(f"{fn}[{h}] stride below the limit", search(fn, e[h], limit=10, stride=9, **kw), -3)
        add(f"{fn}[{h}] limit 0 is every key: stride 49 of 50", search(fn, e[h], limit=0, stride=49, **kw), -3)
        add(f"{fn}[{h}] limit above the keys: stride 49 of 50", search(fn, e[h], limit=1000, stride=49, **kw), -3)
    add("ngsSearchDeviceU8 narrow handle", search("ngsSearchDeviceU8", e["N"]), -3)
    add("ngsSearchDeviceU8 narrow handle, n = 0", search("ngsSearchDeviceU8", e["N"], n=0), -3)
    add("ngsSearchDeviceAsync null ticket", search("ngsSearchDeviceAsync", e["N"], extra=(None,)), -3)
    add("ngsSearchDeviceAsync unknown handle, null ticket", search("ngsSearchDeviceAsync", e["X"], extra=(None,)), -1)
    add("ngsSearchDeviceAsync unbuilt handle, null ticket", search("ngsSearchDeviceAsync", e["E"], extra=(None,)), -2)

    # ---- ngsSimilarityDevice(M) / ngsRerankDevice(M): arguments first, then handle, then built
    def sim(h, off=P, n=4, stride=8, cnt=P, keys=P, v=P):
        return ("ngsSimilarityDevice", (h, P, off, n, stride, cnt, keys, v, None))

    def sim_m(h, off=P, n=4, stride=8, cnt=P, keys=P, metric=0, v=P, t=None):
        return ("ngsSimilarityDeviceM", (h, P, off, n, stride, cnt, keys, metric, v, t, None))

    def rr(h, off=P, n=4, stride=8, cnt=P, keys=P, sc=P, v=P, ms=0.5):
        return ("ngsRerankDevice", (h, P, off, n, stride, cnt, keys, sc, v, ms, None))

    def rr_m(h, off=P, n=4, stride=8, cnt=P, keys=P, sc=P, v=P, t=None, metric=0, ms=0.5):
        return ("ngsRerankDeviceM", (h, P, off, n, stride, cnt, keys, sc, v, t, metric, ms, None))

    for f in (sim, sim_m, rr, rr_m):
        nm = f(0)[0]
        add(f"{nm} unknown handle", f(e["X"]), -1)
        add(f"{nm} unbuilt handle", f(e["E"]), -2)
        add(f"{nm} null offsets", f(e["N"], off=None), -3)
        add(f"{nm} null offsets on an unknown handle", f(e["X"], off=None), -3)
        add(f"{nm} null counts on an unbuilt handle", f(e["E"], cnt=None), -3)
        add(f"{nm} null counts, n = 0", f(e["W"], cnt=None, n=0), -3)
        add(f"{nm} null keys", f(e["N"], keys=None), -3)
        add(f"{nm} null sims", f(e["W"], v=None), -3)
    for f in (sim_m, rr_m):
        nm = f(0)[0]
        add(f"{nm} metric 3", f(e["N"], metric=3), -3)
        add(f"{nm} metric 3 on an unknown handle", f(e["X"], metric=3), -3)
        add(f"{nm} metric 2^32 - 1, n = 0", f(e["W"], metric=0xFFFFFFFF, n=0), -3)
    for f in (rr, rr_m):
        nm = f(0)[0]
        add(f"{nm} NaN minSimilarity", f(e["N"], ms=NAN), -3)
        add(f"{nm} NaN minSimilarity on an unknown handle", f(e["X"], ms=NAN), -3)
        add(f"{nm} NaN minSimilarity, n = 0", f(e["N"], ms=NAN, n=0), -3)
        add(f"{nm} null scores", f(e["N"], sc=None), -3)
        add(f"{nm} stride 4097", f(e["N"], stride=4097), -3)
        add(f"{nm} stride 4097 on an unbuilt handle, n = 0", f(e["E"], stride=4097, n=0), -3)

    # ---- ngsKeyQueriesDevice: the pointers, then handle, built, range, capacity and alignment
    def kq(h, first=0, n=10, b=P, cap=1 << 16, off=P):
        return ("ngsKeyQueriesDevice", (h, first, n, b, cap, off, None))

    add("ngsKeyQueriesDevice unknown handle", kq(e["X"]), -1)
    add("ngsKeyQueriesDevice unbuilt handle", kq(e["E"]), -2)
    add("ngsKeyQueriesDevice unbuilt handle, keys past the end", kq(e["E"], first=40, n=11), -2)
    add("ngsKeyQueriesDevice null offsets", kq(e["N"], off=None), -3)
    add("ngsKeyQueriesDevice null offsets on an unknown handle", kq(e["X"], off=None), -3)
    add("ngsKeyQueriesDevice null bytes with a capacity, unbuilt handle", kq(e["E"], b=None), -3)
    add("ngsKeyQueriesDevice keys past the last key", kq(e["N"], first=40, n=11), -3)
    add("ngsKeyQueriesDevice first key past the last key", kq(e["W"], first=51, n=0), -3)
    add("ngsKeyQueriesDevice first + n wraps 32 bits", kq(e["N"], first=0xFFFFFFFF, n=2), -3)
    add("ngsKeyQueriesDevice capacity one byte short", kq(e["N"], cap=e["ix"].key_query_bytes(0, 10) - 1), -3)
    add("ngsKeyQueriesDevice wide handle, bytes off a 4-byte boundary", kq(e["W"], b=P + 2), -3)

    # ---- ngsSelfJoinDevice: the pointers, then handle, built, range and stride
    def sj(h, first=0, n=10, limit=10, stride=11, cnt=P, keys=P, sc=P):
        return ("ngsSelfJoinDevice", (h, first, n, 0.0, limit, stride, cnt, keys, sc, None))

    add("ngsSelfJoinDevice unknown handle", sj(e["X"]), -1)
    add("ngsSelfJoinDevice unknown handle, keys past the end", sj(e["X"], first=45, n=10), -1)
    add("ngsSelfJoinDevice unbuilt handle", sj(e["E"]), -2)
    add("ngsSelfJoinDevice unbuilt handle, stride below the limit", sj(e["E"], stride=1), -2)
    add("ngsSelfJoinDevice null counts", sj(e["N"], cnt=None), -3)
    add("ngsSelfJoinDevice null counts on an unknown handle", sj(e["X"], cnt=None), -3)
    add("ngsSelfJoinDevice null keys on an unbuilt handle", sj(e["E"], keys=None), -3)
    add("ngsSelfJoinDevice null scores", sj(e["W"], sc=None), -3)
    add("ngsSelfJoinDevice keys past the last key", sj(e["N"], first=45, n=6), -3)
    add("ngsSelfJoinDevice keys past the last key, wide", sj(e["W"], first=50, n=1), -3)
    add("ngsSelfJoinDevice stride 10 below limit + 1", sj(e["N"], limit=10, stride=10), -3)
    add("ngsSelfJoinDevice limit 0 is every key: stride 49 of 50", sj(e["W"], limit=0, stride=49), -3)
    add("ngsSelfJoinDevice stride below the limit, no keys asked for", sj(e["N"], n=0, stride=3), -3)

    # ---- ngsTerm: handle, built, term id, then the buffer
    nt, ntw = e["ix"].size(), e["wix"].size()
    add("ngsTerm unknown handle", ("ngsTerm", (e["X"], 0, P, 64)), -1)
    add("ngsTerm unbuilt handle", ("ngsTerm", (e["E"], 0, P, 64)), -2)
    add("ngsTerm first id past the terms", ("ngsTerm", (e["N"], nt, P, 64)), -3)
    add("ngsTerm id 2^32 - 1, wide", ("ngsTerm", (e["W"], 0xFFFFFFFF, P, 64)), -3)
    add("ngsTerm id past the terms and a null buffer", ("ngsTerm", (e["W"], ntw, None, 64)), -3)
    add("ngsTerm null buffer with a capacity", ("ngsTerm", (e["N"], 0, None, 64)), -3)
    return out


def test_return_codes_of_the_device_entry_points(env):
    L = _native.lib()
    cases = _cases(env)
    assert len(cases) > 120
    wrong = []
    for name, fn, args, want in cases:
        got = getattr(L, fn)(*args)
        if got != want:
            wrong.append(f"{name}: {fn} answered {got}, expected {want}")
    assert not wrong, "\n".join(wrong)
    # nothing was left pending or marked: both libraries still answer
    torch.cuda.synchronize()
    assert len(env["ix"].score_batch([b"KEY NUMBER 07"], 0.0, 3)[0]) == 3
    assert len(env["wix"].score_batch(["KEY NUMBER 07"], 0.0, 3)[0]) == 3
