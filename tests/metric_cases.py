"""Shared material of tests/test_metric_host.py and tests/test_gpu_metric.py: the planted pairs that
tell the metrics apart, and the small device helpers of the GPU tests (torch is imported where they
run, so the CPU tests can import this module)."""
from __future__ import annotations

import numpy as np

import metric_ref
import sim_ref

ALPHA36 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
FILL = 0x7FC0FADE  # a NaN pattern no similarity and no term id has: cells the kernels must not write keep it
GUARD = 64
DEV = "cuda:0"


# ---- planted pairs ----------------------------------------------------------------------------
def no_equal_neighbours(rng, n: int, alpha=ALPHA36) -> list:
    """n characters, no two neighbours equal: every adjacent swap changes the string."""
    out = []
    for _ in range(n):
        c = rng.choice(alpha)
        while out and c == out[-1]:
            c = rng.choice(alpha)
        out.append(c)
    return out


def swapped(q, at) -> list:
    """q with the neighbours (p, p + 1) swapped for every p of `at` (no two of them overlap)."""
    t = list(q)
    for p in at:
        t[p], t[p + 1] = t[p + 1], t[p]
    return t


def swap_positions(rng, m: int) -> list:
    """The swap sets of one query of length m >= 2: the first pair, the last pair, the pairs across the
    64-row block boundaries (rows 63|64, 127|128) where m reaches them, and random sets of one to three."""
    sets = [[0], [m - 2]]
    sets += [[p] for p in (63, 127) if p + 1 < m]
    if m > 129:
        sets.append([63, 127])
    for k in (1, 2, 3):
        for _ in range(2):
            ps = sorted(rng.sample(range(m - 1), min(k, m - 1)))
            ps = [p for i, p in enumerate(ps) if i == 0 or p - ps[i - 1] >= 2]
            sets.append(ps)
    return sets


def swap_pairs(rng, m: int, alpha=ALPHA36, reps: int = 1) -> list:
    """(query, term) pairs (tuples of ints): the term is the query with one to three adjacent swaps of
    differing characters; every second one also has a substitution."""
    out = []
    for _ in range(reps):
        q = no_equal_neighbours(rng, m, alpha)
        fixed = 2 + (m > 64) + (m > 128) + (m > 129)  # the mandated sets stay pure swaps
        for n, at in enumerate(swap_positions(rng, m)):
            t = swapped(q, at)
            if n >= fixed and (n - fixed) % 2:
                p = rng.randrange(m)
                t[p] = rng.choice([c for c in alpha if c != t[p]])
            out.append((tuple(q), tuple(t)))
    return out


def embedded(rng, q, alpha=ALPHA36, lo: int = 1, hi: int = 40) -> tuple:
    """A term that holds q with one substitution, between lo..hi other characters on either side."""
    inner = list(q)
    p = rng.randrange(len(q))
    inner[p] = rng.choice([c for c in alpha if c != inner[p]])
    pre = [rng.choice(alpha) for _ in range(rng.randint(lo, hi))]
    post = [rng.choice(alpha) for _ in range(rng.randint(lo, hi))]
    return tuple(pre + inner + post)


def substring_pairs(rng, m: int, alpha=ALPHA36, reps: int = 2) -> list:
    """(query, term): the query with one substitution sits inside a longer term."""
    out = []
    for _ in range(reps):
        q = tuple(rng.choice(alpha) for _ in range(m))
        out.append((q, embedded(rng, q, alpha)))
    return out


def assert_not_vacuous(swaps, subs):
    """On the model alone: the planted pairs tell the metrics apart, so code that returned Levenshtein
    for every metric could not pass."""
    if swaps:
        qs, ts = [p[0] for p in swaps], [p[1] for p in swaps]
        dl = metric_ref.dist_batch(qs, ts, metric_ref.LEVENSHTEIN)
        do = metric_ref.dist_batch(qs, ts, metric_ref.OSA)
        assert (do <= dl).all()
        share = float((do < dl).mean())
        assert share >= 0.25, f"only {share:.0%} of the planted swap pairs have d_OSA < d_Levenshtein"
    if subs:
        qs, ts = [p[0] for p in subs], [p[1] for p in subs]
        dl = metric_ref.dist_batch(qs, ts, metric_ref.LEVENSHTEIN)
        dp = metric_ref.dist_batch(qs, ts, metric_ref.PARTIAL)
        assert (dp < dl).all(), "a planted substring pair has d_PARTIAL >= d_Levenshtein"


# ---- device helpers (as in tests/test_gpu_sim.py) ------------------------------------------------
def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def ready():
    """The buffers torch filled on its current stream are complete before a call on another stream reads them."""
    import torch
    torch.cuda.current_stream().synchronize()


def pack(queries, cs):
    """Raw queries (sequences of ints) -> device bytes and byte offsets in ngsSearchDevice's layout."""
    import torch
    dt = np.uint8 if cs == 1 else np.uint32
    flat = np.concatenate([np.asarray(q, dtype=dt) for q in queries] + [np.zeros(0, dtype=dt)])
    offs = np.cumsum([0] + [len(q) * cs for q in queries], dtype=np.int64)
    raw = torch.from_numpy(np.frombuffer(flat.tobytes() + bytes(16), dtype=np.uint8).copy()).to(DEV)
    return raw, torch.from_numpy(offs).to(DEV)


def block(counts, keys, stride):
    """counts[n], keys[n][<= stride] -> device counts and key ids at i * stride (the rest 0xEEEEEEEE)."""
    import torch
    n = len(counts)
    k = np.full((n, stride), 0xEEEEEEEE, dtype=np.uint32)
    for i, row in enumerate(keys):
        k[i, :len(row)] = row
    return (torch.from_numpy(np.asarray(counts, dtype=np.uint32).view(np.int32)).to(DEV),
            torch.from_numpy(k.view(np.int32)).to(DEV))


def filled(cells):
    import torch
    return torch.full((cells + GUARD,), FILL, dtype=torch.int32, device=DEV)


def similarity_m(ix, queries, counts, keys, stride, metric, with_terms, cs=1, qbuf=None, stream=None):
    """ngsSimilarityDeviceM -> (sims as u32 bits [n][stride], term ids [n][stride] or None); the guard
    cells behind both outputs and dCounts are checked here."""
    import torch
    n = len(queries)
    raw, off = qbuf if qbuf is not None else pack(queries, cs)
    dn, dk = block(counts, keys, stride)
    dv, dt = filled(n * stride), filled(n * stride) if with_terms else None
    s = stream if stream is not None else torch.cuda.Stream()
    ready()
    ix.similarity_device(raw.data_ptr(), off.data_ptr(), n, stride, dn.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                         s.cuda_stream, metric=metric, d_terms=dt.data_ptr() if with_terms else 0)
    s.synchronize()
    assert np.array_equal(dn.cpu().numpy().view(np.uint32), np.asarray(counts, dtype=np.uint32)), "dCounts written"
    out = []
    for d in (dv, dt):
        if d is None:
            out.append(None)
            continue
        a = d.cpu().numpy().view(np.uint32)
        assert (a[n * stride:] == FILL).all(), "wrote past the block"
        out.append(a[:n * stride].reshape(n, stride))
    return out


def term_table(ix, wide=False):
    """{term (tuple of ints): term id} through ngsTerm, every id 0 .. size() - 1."""
    out = {}
    for t in range(ix.size()):
        s = ix.term(t)
        u = tuple(sim_ref.units(s, wide))
        assert u not in out, f"term {t} repeats term {out.get(u)}"
        out[u] = t
    return out


def key_term_sets(ix, words, row_size=1, weights=None, wide=False):
    """key id -> the key's normalised terms (the model's), through the key strings of the index."""
    kt = sim_ref.key_terms(words, row_size, weights, wide)
    out = [kt[tuple(sim_ref.units(ix.key(k), wide))] for k in range(ix.num_keys())]
    assert len(out) == len(kt)
    return out


def expect_m(queries, counts, keys, stride, key_terms, term_ids, metric, valid=sim_ref.DEFAULT_VALID, wide=False):
    """The blocks ngsSimilarityDeviceM must leave: (sim bits, term ids) where r < min(count, stride),
    FILL elsewhere."""
    n = len(queries)
    want = np.full((n, stride), FILL, dtype=np.uint32)
    want_t = np.full((n, stride), FILL, dtype=np.uint32)
    pairs, cells = [], []
    for i, q in enumerate(queries):
        for r in range(min(counts[i], stride)):
            k = int(keys[i][r])
            pairs.append((tuple(q), key_terms[k] if k < len(key_terms) else None))
            cells.append((i, r))
    sims, best = metric_ref.record_sims(pairs, metric, term_ids, valid, wide)
    for (i, r), b, t in zip(cells, bits(sims), best):
        want[i, r] = b
        want_t[i, r] = metric_ref.NO_TERM if t is None else term_ids[t]
    return want, want_t


def check_cells(got, want, where):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{where}: query {bad[0][0]} record {bad[0][1]}: got {got[tuple(bad[0])]:#x}, "
                           f"want {want[tuple(bad[0])]:#x}")
