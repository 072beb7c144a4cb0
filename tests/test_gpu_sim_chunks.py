"""scoreBatchSim across its chunk boundary: a call whose queries x limit pass 2^22 records is run in
chunks of floor(2^22 / limit) queries. 1,100 queries at limit 4,096 on 4,200 keys that all share a word
(so that every query has 4,096 records at threshold 0) make 4.5 M records: chunks of 1,024 and 76.

The whole batch must equal the same call on queries[:1024] and queries[1024:] put together, and its
first 20 queries the model of sim_ref.py / metric_ref.py on the oracle's answers. min_similarity 0.8
leaves a few dozen records per query (two edits in eleven characters), so the host side stays cheap.
"""
import random

import numpy as np
import pytest

import metric_ref
import sim_ref
from oracle_py import OracleIndex

import stringsearchlib_amd as ssl

pytestmark = pytest.mark.gpu

LIMIT, NQ, CUT, MODEL = 4096, 1100, 1024, 20
MIN_SIM = 0.8


def bits(x):
    return int(np.asarray([x], dtype=np.float32).view(np.uint32)[0])


@pytest.fixture(scope="module")
def lib():
    rng = random.Random(0xC4)
    tails = set()
    while len(tails) < 4200:
        tails.add(bytes(rng.choice(b"ABCDE") for _ in range(7)))
    words = [b"ZQX " + t for t in sorted(tails)]
    rng.shuffle(words)
    queries = []
    for i in range(NQ):
        w = bytearray(rng.choice(words))
        for _ in range(i % 3):  # none, one or two substitutions in the tail
            w[rng.randrange(4, 11)] = rng.choice(b"ABCDEabcde")
        queries.append(bytes(w))
    assert (2 ** 22) // LIMIT == CUT and NQ * LIMIT > 2 ** 22 and len(words) > LIMIT
    ix = ssl.StringIndex(words, 1)
    oi = OracleIndex(words, 1, None)
    answers = [oi.score(q, 0.0, LIMIT) for q in queries[:MODEL]]
    assert all(len(a) == LIMIT for a in answers)  # every query fills its 4,096 records
    yield ix, words, queries, answers
    ix.dispose()


def model(words, queries, answers, metric, with_terms):
    """[(key, score bits, sim bits[, term])] per query: one term per key, the normalised key."""
    kt = sim_ref.key_terms(words)
    pairs = [(tuple(q), kt[tuple(k)]) for q, a in zip(queries, answers) for k, _ in a]
    lev = metric == metric_ref.LEVENSHTEIN
    sims = sim_ref.record_sims(pairs) if lev else metric_ref.record_sims(pairs, metric)[0]
    out, o = [], 0
    for a in answers:
        terms = [bytes(next(iter(kt[tuple(k)]))) for k, _ in a]
        ks, ss, vs, ts = metric_ref.rerank([k for k, _ in a], [s for _, s in a], list(sims[o:o + len(a)]), terms, MIN_SIM)
        out.append([(k, bits(s), bits(v)) + ((t,) if with_terms else ()) for k, s, v, t in zip(ks, ss, vs, ts)])
        o += len(a)
    return out


def as_bits(rows):
    return [[(r[0], bits(r[1]), bits(r[2])) + tuple(r[3:]) for r in row] for row in rows]


@pytest.mark.parametrize("metric, with_terms", [(None, False), ("osa", True)])
def test_two_chunks_equal_the_two_calls_and_the_model(lib, metric, with_terms):
    ix, words, queries, answers = lib
    kw = {} if metric is None else {"metric": metric, "with_terms": with_terms}
    whole = ix.score_batch_sim(queries, 0.0, LIMIT, MIN_SIM, **kw)
    parts = ix.score_batch_sim(queries[:CUT], 0.0, LIMIT, MIN_SIM, **kw) + \
        ix.score_batch_sim(queries[CUT:], 0.0, LIMIT, MIN_SIM, **kw)
    assert len(whole) == NQ
    kept = sum(map(len, whole))
    assert 0 < kept < 100 * NQ, kept  # the filter bit, and left something on both sides of the cut
    assert any(whole[CUT:]) and all(len(r[0]) == (4 if with_terms else 3) for r in whole if r)
    assert as_bits(whole) == as_bits(parts)
    want = model(words, queries[:MODEL], answers, metric_ref.METRICS[metric or "levenshtein"], with_terms)
    assert as_bits(whole[:MODEL]) == want
