"""ngsMatchDevice on the GPU: the fabricated blocks of tests/match_cases.py through a caller-side loop of
rounds, in one block and cut into several, against the sequential greedy of tests/match_ref.py.
Every comparison is exact; no index is needed."""
import numpy as np
import pytest

import match_cases
import match_ref

import stringsearchlib_amd as ssl
from stringsearchlib_amd import _native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
FILL32 = 0x5A5AA5A5
FILL64 = 0x5A5AA5A55A5AA5A5
NO_MATCH = match_ref.NO_MATCH
CASES = match_cases.cases()


def dev_u32(a, guard=True):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if guard:
        a = np.concatenate([a, np.full(GUARD, FILL32, dtype=np.uint32)])
    return torch.from_numpy(a.view(np.int32).copy()).to(DEV)


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.current_stream().synchronize()


class State:
    """The match arrays, the bids and the pair count, each with guard cells behind it and junk inside."""

    def __init__(self, n_a, n_b):
        self.n_a, self.n_b = n_a, n_b
        self.ma = dev_u32(np.full(n_a, 12345, dtype=np.uint32))
        self.mb = dev_u32(np.full(n_b, 54321, dtype=np.uint32))
        self.bids = torch.full((n_b + GUARD,), FILL64, dtype=torch.int64, device=DEV)
        self.matched = dev_u32(np.full(1, 777, dtype=np.uint32))
        sync()

    def step(self, block, **flags):
        dn, dk, dv, n, stride, first = block
        ssl.StringIndex.match_device(dn.data_ptr() if n else 0, dk.data_ptr() if n else 0, dv.data_ptr() if n else 0,
                                     n, stride, first, self.ma.data_ptr(), self.n_a, self.mb.data_ptr(), self.n_b,
                                     self.bids.data_ptr(), self.matched.data_ptr(), stream=stream(), **flags)

    def pairs(self):
        sync()
        return int(host_u32(self.matched)[0])

    def result(self):
        sync()
        ma, mb, bids, m = host_u32(self.ma), host_u32(self.mb), self.bids.cpu().numpy(), host_u32(self.matched)
        assert (ma[self.n_a:] == FILL32).all(), "dMatchA written past nA"
        assert (mb[self.n_b:] == FILL32).all(), "dMatchB written past nB"
        assert (bids[self.n_b:] == FILL64).all(), "dBids written past nB"
        assert (m[1:] == FILL32).all(), "written behind *dMatched"
        return ma[:self.n_a].tolist(), mb[:self.n_b].tolist(), int(m[0])


def dev_block(counts, keys, values, n, stride, first):
    return (dev_u32(counts), dev_u32(keys), dev_u32(values.view(np.uint32)), n, stride, first)


def check_inputs_untouched(block, counts, keys, values):
    dn, dk, dv = block[:3]
    for t, a in ((dn, counts), (dk, keys), (dv, values.view(np.uint32))):
        g = host_u32(t)
        assert (g[:len(a)] == a).all() and (g[len(a):] == FILL32).all(), "the block was written"


def run_rounds(state, blocks, limit):
    """Rounds over the blocks until one adds nothing -> the pairs added by each round."""
    none = (None, None, None, 0, 1, 0)
    state.step(none, init=True, begin=False, bid=False, accept=False)
    adds, before = [], 0
    assert state.pairs() == 0
    while True:
        if len(blocks) == 1:
            state.step(blocks[0])  # BEGIN | BID | ACCEPT
        else:
            for j, b in enumerate(blocks):
                state.step(b, begin=j == 0, accept=False)
            for b in blocks:
                state.step(b, begin=False, bid=False)
        now = state.pairs()
        adds.append(now - before)
        before = now
        if adds[-1] == 0:
            return adds
        assert len(adds) <= limit, "the rounds do not end"


def no_live_edge(rows, ma, mb):
    return all(ma[a] != NO_MATCH or all(mb[b] != NO_MATCH for _, b in es) for a, es in rows.items())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rounds_give_the_greedy_matching(case):
    name, n_a, n_b, first, n, stride, counts, keys, values = case
    rows = match_ref.block_rows(counts, keys, values.view(np.uint32), n, stride, first, n_a, n_b)
    want_a, want_b = match_ref.greedy(n_a, n_b, rows)
    pairs = sum(1 for b in want_a if b != NO_MATCH)
    assert pairs > 0
    # one block
    block = dev_block(counts, keys, values, n, stride, first)
    st = State(n_a, n_b)
    adds = run_rounds(st, [block], pairs + 1)
    ma, mb, m = st.result()
    assert ma == want_a and mb == want_b, name
    assert m == pairs == sum(adds)
    assert all(a > 0 for a in adds[:-1]), f"{name}: a round with live edges added nothing: {adds}"
    assert no_live_edge(rows, ma, mb)
    check_inputs_untouched(block, counts, keys, values)
    if name == "chain":
        assert len(adds) == 71 and adds[:-1] == [1] * 70
    if name == "contention":
        assert len(adds) in (2, 3) and adds[0] >= 1
    # a round on the complete matching changes nothing
    st.step(block)
    assert st.result() == (want_a, want_b, pairs)


@pytest.mark.parametrize("case", CASES[:5], ids=[c[0] for c in CASES[:5]])
def test_blocks_cut_at_random_rows_give_the_one_block_result(case):
    name, n_a, n_b, first, n, stride, counts, keys, values = case
    rows = match_ref.block_rows(counts, keys, values.view(np.uint32), n, stride, first, n_a, n_b)
    want_a, want_b = match_ref.greedy(n_a, n_b, rows)
    pairs = sum(1 for b in want_a if b != NO_MATCH)
    for seed in (1, 2):
        cuts = match_cases.cuts_of(n, seed * 1000 + stride)
        assert len(cuts) >= 5 and any(a == b for a, b in zip(cuts, cuts[1:]))
        blocks = [dev_block(counts[a:b], keys[a * stride:b * stride], values[a * stride:b * stride], b - a, stride,
                            first + a) for a, b in zip(cuts, cuts[1:])]
        st = State(n_a, n_b)
        adds = run_rounds(st, blocks, pairs + 1)
        assert st.result() == (want_a, want_b, pairs), (name, cuts)
        assert all(a > 0 for a in adds[:-1])


def test_init_alone_sets_the_arrays():
    st = State(100, 37)
    st.step((None, None, None, 0, 5, 0), init=True, begin=False, bid=False, accept=False)
    ma, mb, m = st.result()
    assert ma == [NO_MATCH] * 100 and mb == [NO_MATCH] * 37 and m == 0
    assert (st.bids.cpu().numpy()[:37] == FILL64).all()  # BEGIN clears the bids, INIT does not
    st.step((None, None, None, 0, 5, 0), init=False, begin=True, bid=True, accept=True)
    assert st.result() == (ma, mb, 0) and (st.bids.cpu().numpy()[:37] == 0).all()
    # no sources or no targets: nothing to match, nothing read
    L = _native.lib()
    one = dev_u32(np.zeros(1, dtype=np.uint32))
    assert L.ngsMatchDevice(one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 1, 0, None, 0, st.mb.data_ptr(), 37,
                            st.bids.data_ptr(), st.matched.data_ptr(), 15, None) == 0
    assert L.ngsMatchDevice(one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 1, 0, st.ma.data_ptr(), 100, None, 0,
                            None, st.matched.data_ptr(), 15, None) == 0
    torch.cuda.synchronize()
    assert st.result() == ([NO_MATCH] * 100, [NO_MATCH] * 37, 0)
