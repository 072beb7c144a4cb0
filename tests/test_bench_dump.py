"""bench.py --dump-outputs on CPU: dump_outputs over a step loop's gather buffers.

What it writes is what the last timed step left in its buffer: the counts of the whole batch, and
keys / scores of every query (batch <= 16,384) or of a fixed seeded sample (larger batches), with
the slots past a query's count blanked. Checked on a batch of each kind, with the buffers the loop
did not write last filled with other values."""
import types

import numpy as np
import pytest
import torch

import bench
from stringsearchlib_amd import shard


def _loop(B, stride, nbuf, nstep, seed):
    g = torch.Generator().manual_seed(seed)
    gbs = [shard.PackedGather(B, stride, B, torch.device("cpu")) for _ in range(nbuf)]
    for gb in gbs:
        gb.counts.copy_(torch.randint(0, stride + 1, (B,), generator=g, dtype=torch.int32))
        gb.keys.copy_(torch.randint(0, 10_000_000, (B * stride,), generator=g, dtype=torch.int32))
        gb.scores.copy_(torch.rand(B * stride, generator=g) * 100)
    return types.SimpleNamespace(gbs=gbs, nbuf=nbuf, nstep=nstep, B=B, stride=stride)


@pytest.mark.parametrize("B,stride", [(300, 7), (bench.DUMP_ROWS + 1000, 3)])
def test_dump_outputs_last_buffer(tmp_path, B, stride):
    loop = _loop(B, stride, nbuf=3, nstep=8, seed=B)
    last = loop.gbs[(8 - 1) % 3]
    bench.dump_outputs(str(tmp_path / "a"), loop)
    bench.dump_outputs(str(tmp_path / "b"), loop)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("counts", "rows", "keys", "scores")}
    for n, a in got.items():  # the same files again: the sample is fixed
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{n}.npy")), n
    assert got["counts"].dtype == np.float64 and got["keys"].dtype == np.float64
    assert got["scores"].dtype == np.float32 and got["rows"].dtype == np.float64
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    counts = last.counts.numpy()
    assert np.array_equal(got["counts"], counts.astype(np.float64))
    rows = got["rows"].astype(np.int64)
    R = min(B, bench.DUMP_ROWS)
    assert rows.shape == (R,) and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < B
    if B <= bench.DUMP_ROWS:
        assert np.array_equal(rows, np.arange(B))
    keys = last.keys.numpy().reshape(B, stride)[rows]
    scores = last.scores.numpy().reshape(B, stride)[rows]
    assert got["keys"].shape == (R, stride) and got["scores"].shape == (R, stride)
    for r in range(R):
        n = counts[rows[r]]
        assert np.array_equal(got["keys"][r, :n], keys[r, :n].astype(np.float64))
        assert np.array_equal(got["scores"][r, :n], scores[r, :n])
        assert np.all(got["keys"][r, n:] == -1) and np.all(got["scores"][r, n:] == 0)
