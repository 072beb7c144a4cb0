"""bench.py's command line on the GPU, at a small shape (20,000 rows, 300 queries, 3 steps).

A plain run times the steps it is asked for and prints the headline line only; --dump-outputs
writes the last timed step's results, the same from run to run and equal to the oracle's answers
(keys by their strings, scores by their bits); --full adds the roofline and the drop-in legs."""
import ctypes as C
import json

import numpy as np
import pytest

import bench
from oracle_py import lib as olib
from tiecheck import bits

from stringsearchlib_amd import _native

pytestmark = pytest.mark.gpu

ROWS, BATCH, STEPS = 20_000, 300, 3
ARGS = ["--rows", str(ROWS), "--batch", str(BATCH), "--steps", str(STEPS), "--warmup", "1"]
HEADLINE = {"metric": bench.METRIC, "unit": "Mqueries/s", "higher_is_better": True, "dtype": "u32", "steps": STEPS,
            "n_gpus": 1}


def _run(capsys, extra):
    bench.main(ARGS + extra)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for k, v in HEADLINE.items():
        assert line[k] == v, (k, line[k])
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value is queries over the timed steps' time: consistent with ms_per_step (both rounded to 4 places)
    assert line["value"] == pytest.approx(BATCH / line["ms_per_step"] / 1e3, rel=1e-2)
    return line


def test_plain_run_dumps_the_oracles_answers(capsys, tmp_path):
    line = _run(capsys, ["--dump-outputs", str(tmp_path / "a")])
    assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None
    assert "dropin" not in line["detail"]
    _run(capsys, ["--dump-outputs", str(tmp_path / "b")])
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("counts", "rows", "keys", "scores")}
    for n, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{n}.npy")), n
    assert np.array_equal(got["rows"], np.arange(BATCH))

    cfg = bench.CONFIGS["c3"]
    corpus = bench.Corpus(ROWS)
    raw, offs = corpus.queries(BATCH)
    qs = [raw[offs[i]:offs[i + 1]] for i in range(BATCH)]
    O, L = olib(), _native.lib()
    oh = O.ngo_build(corpus.words, corpus.n_words, 1, corpus.weights)
    limit = cfg["limit"]
    counts = (C.c_uint32 * BATCH)()
    keys = (C.c_uint32 * (BATCH * limit))()
    scores = (C.c_float * (BATCH * limit))()
    O.ngo_search_batch(oh, (C.c_char_p * BATCH)(*qs), BATCH, cfg["threshold"], limit, counts, keys, scores, limit, 8)
    h = bench.build_index(corpus, True, 0)  # the key strings of the dumped ids
    assert got["counts"].tolist() == list(counts) and sum(counts) > 0
    for i in range(BATCH):
        for j in range(counts[i]):
            ln = C.c_uint32()
            want = C.string_at(O.ngo_key(oh, keys[i * limit + j], C.byref(ln)), ln.value)
            assert C.string_at(L.ngsKey(h, int(got["keys"][i, j]))) == want, (i, j)
            assert bits(float(got["scores"][i, j])) == bits(scores[i * limit + j]), (i, j)
        assert np.all(got["keys"][i, counts[i]:] == -1)
    L.dispose(h)
    O.ngo_free(oh)
    corpus.free()


def test_full_run_adds_roofline_and_dropin(capsys):
    line = _run(capsys, ["--full", "--no-cpu-baseline"])
    assert line["full"] is True and line["cpu_baseline"] is None
    assert line["roofline"]["achieved"] > 0 and line["roofline"]["alg_bytes_per_launch"] > 0
    assert line["detail"]["results_per_query"] > 0 and set(line["detail"]["paths"]) >= {"tier1a_finished", "general"}
    assert line["detail"]["dropin"]["scorebatch_mqs"] > 0 and line["detail"]["dropin"]["c1_score_us_p50"] > 0
