"""The removal plans of the dead-key end-to-end tests (tests/test_gpu_set_dead.py) over the libraries of
tests/set_corpus.py. A plan is a list of master keys (key strings) to remove; the host test
(tests/test_set_dead_host.py) checks on the CPU that the oracle over the rows left flags none of the
narrow queries as ambiguous, with an allowance of zero: a plan that trips it gets another seed."""
from __future__ import annotations

import functools
import random

import set_corpus

ROW = set_corpus.ROW
PLAN_A_SEED = 101
WIDE_A_SEED = 103
PLANS = ("a", "b", "c", "d", "e")


def family():
    """The narrow tie family's master keys by rank for TIE_QUERY: one score and one length, so by first
    appearance, which is the order of their numbers."""
    return [set_corpus.TIE_QUERY + b"%03d" % n for n in range(set_corpus.FAMILY)]


@functools.lru_cache(maxsize=None)
def plan(name: str):
    """The master keys plan `name` removes from set_corpus.narrow()."""
    words, _, cuts = set_corpus.narrow()
    masters = words[::ROW]
    if name == "a":    # a tenth of the keys at random
        return tuple(random.Random(PLAN_A_SEED).sample(masters, len(masters) // 10))
    if name == "b":    # every second member of the tie family: a tie class is cut at another place
        return tuple(family()[::2])
    if name == "c":    # the keys the exact-match queries promote to 100
        have = set(masters)
        return tuple(dict.fromkeys(q for q in set_corpus.narrow_queries() if q in have))
    if name == "d":    # both keys of the first member: a member wholly dead
        return tuple(masters[cuts[0]:cuts[1]])
    if name == "e":    # the first 150 of the family by rank: TIE_QUERY at limit 10 meets more dead records
        return tuple(family()[:150])  # than the first over-fetch holds
    raise KeyError(name)


def live_rows(words, weights, removed):
    """(words, weights) of the rows whose master key is not in `removed`."""
    gone = set(removed)
    keep = [r for r in range(len(words) // ROW) if words[ROW * r] not in gone]
    w = [words[ROW * r + j] for r in keep for j in range(ROW)]
    wt = [weights[ROW * r + j] for r in keep for j in range(ROW)]
    return w, wt


@functools.lru_cache(maxsize=None)
def wide_plan():
    """A tenth of the wide library's keys at random, and every second member of the wide tie family."""
    words, _, _ = set_corpus.wide()
    masters = words[::ROW]
    out = random.Random(WIDE_A_SEED).sample(masters, len(masters) // 10)
    out += [set_corpus.WIDE_TIE_QUERY + "%03d" % n for n in range(0, set_corpus.WIDE_FAMILY, 2)]
    return tuple(dict.fromkeys(out))
