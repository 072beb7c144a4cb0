"""The legs of tests/test_gpu_ref_fuzz.py, checked without a GPU (CPU).

tests/ref_fuzz_legs.py drives an index through `score`, `search`, `score_batch`, `size`, `lib_size`
and `key`. Here the index is the oracle itself behind that interface, which must pass every leg on all
three streams, and three deliberately wrong versions of it, each of which the legs must catch:

* one that drops the last result when limit >= the number of keys;
* one that raises one score by one ulp;
* one that swaps two results of a (score, length) tie with different keys: the exact comparison
  with the oracle must catch it, and the tie-aware comparison with the reference must accept it,
  since the reference leaves that order open.

So a subtly wrong kernel cannot pass the GPU legs.
"""
import pytest

import ref_fuzz_legs as legs
from tiecheck import bits, f32

STREAMS = list(legs.rf.SPECS)


def run(name, make, **kw):
    """Both legs over every library of the stream; the tally."""
    tally = legs.Tally()
    for L in legs.libraries(name):
        idx = make(L.words, L.row, L.weights)
        try:
            legs.single_calls(L, idx, tally, **kw)
            legs.batches(L, idx, tally, **kw)
        finally:
            idx.dispose()
    return tally


class DropsLast(legs.OracleBacked):
    """Loses the last result whenever the limit does not cut the answer."""

    def score(self, q, thr, limit):
        res = super().score(q, thr, limit)
        return res[:-1] if limit >= self.oi.n_keys() else res


class OneUlpUp(legs.OracleBacked):
    """The first result's score one ulp away from zero."""

    def score(self, q, thr, limit):
        res = super().score(q, thr, limit)
        return [(res[0][0], f32(bits(res[0][1]) + 1))] + res[1:] if res else res


class SwapsTie(legs.OracleBacked):
    """The first two neighbours with equal score bits and key lengths, swapped."""

    def score(self, q, thr, limit):
        res = super().score(q, thr, limit)
        for i in range(len(res) - 1):
            (k1, s1), (k2, s2) = res[i], res[i + 1]
            if bits(s1) == bits(s2) and len(k1) == len(k2) and k1 != k2:
                res[i], res[i + 1] = res[i + 1], res[i]
                break
        return res


@pytest.mark.parametrize("name", STREAMS)
def test_oracle_backed_index_passes_every_leg(name):
    tally = run(name, legs.OracleBacked)
    print(f"{name}: {tally}")
    spec = legs.rf.SPECS[name]
    n_queries = sum(len(L.qt) for L in legs.libraries(name))
    assert tally.singles == n_queries * len(spec["limits"])
    assert tally.vs_reference > tally.cases // 4 and tally.batch_queries >= legs.BATCH_MIN * tally.batches > 0
    # the order-dependent cases of the stream, once per leg (test_ref_fuzz.py counts the same ones)
    assert tally.order_dependent == 2 * sum(amb for L in legs.libraries(name) for qi, (_, thr) in enumerate(L.qt)
                                            for limit in L.limits for _, amb in [L.expected[qi, bits(thr), limit]])


@pytest.mark.parametrize("name", STREAMS)
@pytest.mark.parametrize("wrong", [DropsLast, OneUlpUp])
def test_wrong_answers_are_caught(name, wrong):
    with pytest.raises(AssertionError):
        run(name, wrong)
    with pytest.raises(AssertionError):  # by the reference's recorded answers alone, too
        run(name, wrong, oracle=False)


@pytest.mark.parametrize("name", STREAMS)
def test_swapped_tie_is_caught_by_the_oracle_and_accepted_by_the_reference(name):
    with pytest.raises(AssertionError, match="vs oracle"):
        run(name, SwapsTie)
    tally = run(name, SwapsTie, oracle=False)
    assert tally.vs_reference > 0
