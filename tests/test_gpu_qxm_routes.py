"""msc_score_multi's routes and results against a recorded table. tools/qxm_routes.py runs a fixed list of small calls -- every route of the
call (matrix cores, digest, ring, raw tiles, queued sparse passes, per-query), one to three blocks, blocks that decline the matrix cores, slot
lists and ranges -- and prints per call the kernel it named, its launches, whether close counts were kept and a SHA-256 of each output array.
tests/golden/qxm_routes.json holds those lines as the library printed them before msc_score_multi became a block plan with one function per
route: a fresh run must print the same. (A process of its own: the library reads its switches once per process, and the rank lists of a sparse
set are built at the third call that asks for them, so the table is reproducible only from a fresh context.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_routes_and_results_match_the_recorded_table():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "qxm_routes.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    got = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    want = [json.loads(ln) for ln in open(os.path.join(ROOT, "tests", "golden", "qxm_routes.json")).read().splitlines()]
    assert [g["case"] for g in got] == [w["case"] for w in want]
    for g, w in zip(got, want):
        assert g == w, (w["case"], {k: (g[k], w[k]) for k in w if g[k] != w[k]})


def test_slow_model_sums_match_the_per_query_passes():
    """the three `--feat slow` calls of the table: their weighted sums hold the two FP64 divergence sums and are left out of the hashes, so
    they are held here to one 1 x M pass per query, with the tolerance of the divergence tests (tests/test_gpu_qxm_direct.py)"""
    import numpy as np
    from meshclust2_amd import api, synth
    rtol, atol = 1e-9, 1e-13
    ctx = api.Context(0)
    slow = api.Feature.from_text(ctx, open(os.path.join(ROOT, "tests", "golden", "weights_cfg5_k9.txt")).read(), 0)
    seqs, _ = synth.families(5308, 140, 1000, family=5, length_jitter=100)
    hs = api.HistogramSet(ctx, 9, 8, len(seqs))
    hs.build(seqs)
    for nq in (2, 65, 130):
        qs = (np.arange(nq, dtype=np.uint32) * 3) % len(seqs)
        multi = api.score_multi(ctx, slow, hs, None, hs, qs, m=len(seqs), want=("sum", "csum", "close"))
        for i in sorted(set(range(0, nq, 7)) | {nq - 1}):
            single = slow.compute(hs, None, hs, int(qs[i]), m=len(seqs))
            for key in ("sum", "csum"):
                assert np.all(np.abs(multi[key][i] - single[key]) <= atol + rtol * np.abs(single[key])), (nq, i, key)
            assert np.array_equal(multi["close"][i], (np.round(single["csum"]) > 0).astype(np.uint8)), (nq, i)
    ctx.close()


def test_flag_routes_and_results_match_the_recorded_table():
    """the second table of tools/qxm_routes.py (--flags): calls that ask for the close flags alone with an earth_movers_distance model -- the
    bound tail, the folded tail, a folded block's second run, the dense walk, one stream, no timing events, a block that is not queued, fewer
    than 64 pairs, mirrors from lists. tests/golden/qxm_flag_routes.json holds the lines (kernel, launches, SHA-256 of flags and counts,
    msc_last_emd_walk, msc_last_fold_screen) of the library before run_matrix became a driver over stage functions. (A process of its own,
    as the first table: the switches are read once per process, and a model remembers its overflows.)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "qxm_routes.py"), "--flags"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    got = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    want = [json.loads(ln) for ln in open(os.path.join(ROOT, "tests", "golden", "qxm_flag_routes.json")).read().splitlines()]
    assert [g["case"] for g in got] == [w["case"] for w in want]
    for g, w in zip(got, want):
        assert g == w, (w["case"], {k: (g[k], w[k]) for k in w if g[k] != w[k]})
