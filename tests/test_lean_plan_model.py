"""The main tier-1a launch's planner (lean_query_g) on the CPU: tests/sanitize/lean_plan_driver.cpp, its
own main, built with g++ from ngs_common.h (the HIP headers on the host side only; no sanitizer).

Lane apportionment (group_share / group_rem_key / group_quota, the functions the kernel calls), over
4,000 random length vectors (1..64 lists, lengths 1..10^6 at every magnitude), one list holding 99 % of
the postings at every list count, all lengths equal, and 63 and 64 lists: every quota is at least 1,
the quotas sum to exactly 64, each is the floor of the exact share or one more, and with up to 32 lists
no list has more than twice the ideal P / 64 postings per lane.

The part cut, restated on the host over random sorted lists and their skip tables (4..32 buckets, up to
63 lists, sparse and dense, two lists in 30 % of the terms, empty leading and trailing buckets, the
halved cap of cmin 2): the parts tile the term ids in order, every posting of every list is in exactly
one part, no fast-path part has more chunks of a list than its cap, each part is the widest that fits,
and the entry limit the kernel compares against (part_entry_limit) is the chunk rule.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include():
    for root in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    raise AssertionError("hip/hip_runtime.h not found (ROCM_PATH)")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_lane_quotas_and_greedy_cut_on_the_host(tmp_path):
    exe = str(tmp_path / "lean_plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                    "-isystem", _hip_include(), "-I", os.path.join(ROOT, "stringsearchlib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "lean_plan_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-2000:]}"
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok", p.stdout[-2000:]
    assert lines[0] == f"quota vectors checked: {4000 + 63 + 64 * 4 + 400}" and lines[1] == "cuts checked: 300", p.stdout
