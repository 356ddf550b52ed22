"""The routes and results of the 1 x M calls against a recorded table. tools/score_routes.py runs a fixed list of small calls -- every pass
kernel of run_score (k_pair_tiles, k_pair_tiles_wide, the merge kernels, k_pair_ranks_1xm, k_pair_ranks_items), every form of the divergence
sums and of the group statistics, the switches that are read on every call, the window call, m = 0 and a slot list of two chunks -- and prints
per call the kernel it named, its launches, its status and a SHA-256 of each output array. tests/golden/score_routes.json holds those lines as
the library printed them before run_score became a route chosen in one place and one function per stage: a fresh run must print the same.
(The last two lines, the window call over a small dense set with the fused and the unfused reduce, were recorded when those cases joined the
table; the 91 lines in front of them are the earlier table's, byte for byte.)
(A process of its own: the rank lists of a set are built at the third pass that asks for them, so the table is reproducible only from a fresh
context. Outputs that hold the two FP64 divergence sums are not in the table; tests/test_gpu_ranks_pass.py and tests/test_gpu_parity.py hold
them to the oracle.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_routes_and_results_match_the_recorded_table():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "score_routes.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    got = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    want = [json.loads(ln) for ln in open(os.path.join(ROOT, "tests", "golden", "score_routes.json")).read().splitlines()]
    assert [g["case"] for g in got] == [w["case"] for w in want]
    for g, w in zip(got, want):
        assert g == w, (w["case"], {k: (g[k], w[k]) for k in w if g[k] != w[k]})
