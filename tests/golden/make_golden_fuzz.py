#!/usr/bin/env python3
"""Records the reference's answers to the seeded cases of tests/test_ref_fuzz.py.

Needs the compiled reference (``make -C oracle ref`` -> oracle/_ref/libStringSearchLib.so). Runs
each test's case stream against it and writes tests/golden/fuzz/<name>.json: per query, in case
order, the query, the reference's full (limit 0) answer as [key, fp32 bits] pairs and its number
of results at each limit of the case. The test reads them back wherever the reference is absent.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]

import test_ref_fuzz as t  # noqa: E402


def main():
    os.makedirs(t.RECORDED, exist_ok=True)
    for name, spec in t.SPECS.items():
        ref = t.RecordingReference()
        cases, ambiguous, failures = t.fuzz(ref, **spec)
        assert not failures, failures[0]
        path = os.path.join(t.RECORDED, name + ".json")
        with open(path, "w") as f:
            json.dump({"source": "nGramSearch/dllmain.cpp (oracle/_ref/libStringSearchLib.so), score() per query",
                       "seed": spec["seed"], "limits": spec["limits"], "queries": ref.queries},
                      f, separators=(",", ":"))
        print(f"{path}: {len(ref.queries)} queries, {cases} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
