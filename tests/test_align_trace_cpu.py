"""msc_align_pairs_trace without a device. (1) tests/align_trace_util.py, the numpy restatement of DESIGN.md 4.6h the GPU tests lean on, is held
to the reference's own triples (tests/golden/align_pairs.npz) and to the section's invariants through a replay that shares nothing with it;
(2) tests/golden/align_trace.npz is what the restatement gives today; (3) tests/align_trace_schedule_check.cpp replays the forward kernel's
schedule, its direction stores and both walks serially over csrc/msc_align.h and csrc/msc_align_trace.h -- the text the kernels compile -- in
a stand-alone program built with the address and undefined-behaviour sanitizers, and compares its runs with the restatement's."""
import os
import subprocess

import numpy as np
import pytest

import align_trace_util
import align_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = align_trace_util.SMALL


@pytest.fixture(scope="module")
def small():
    """the fixture's pairs of at most 40 000 cells under its three parameter sets, traced once"""
    fx = align_util.Fixture()
    sel = np.nonzero(fx.cells() <= SMALL)[0]
    firsts, seconds = [fx.seqs[i] for i in fx.first[sel]], [fx.seqs[i] for i in fx.second[sel]]
    return fx, sel, firsts, seconds, [align_trace_util.trace_many(firsts, seconds, params) for params in fx.params]


def test_the_restatements_triples_are_the_references_and_its_cigars_replay_to_them(small):
    fx, sel, firsts, seconds, traced = small
    assert sel.size >= 150
    for s, params in enumerate(fx.params):
        triples, ops, real = traced[s]
        assert np.array_equal(triples, fx.result[s][sel]), params.tolist()
        assert real.all(), "the fixture's small pairs have real paths under its three sets"
        for p in range(sel.size):
            score, columns, same = align_trace_util.replay(ops[p], firsts[p], seconds[p], params)
            assert (score, columns, same) == tuple(triples[p]), (params.tolist(), int(sel[p]), align_trace_util.cigar_string(ops[p]))


def test_the_counts_hold_on_paths_that_are_not_real():
    """unrelated pairs under parameters that let the reference's finite minus infinity win: the columns and the '=' columns still hold"""
    rs = np.random.RandomState(11)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    firsts = [letters[rs.randint(0, 4, int(rs.randint(1, 121)))].tobytes() for _ in range(120)]
    seconds = [letters[rs.randint(0, 4, int(rs.randint(1, 121)))].tobytes() for _ in range(120)]
    unreal = 0
    for params in ((1, -1, 2, 1), (1, 1, 0, 0), (0, 0, 1, 1)):
        triples, ops, real = align_trace_util.trace_many(firsts, seconds, params)
        assert np.array_equal(triples, align_util.align_many(firsts, seconds, params))
        for p in range(len(firsts)):
            score, columns, same = align_trace_util.replay(ops[p], firsts[p], seconds[p], params)
            assert columns == triples[p, 1] and (params[0] == params[1] or same == triples[p, 2])
            assert not real[p] or score == triples[p, 0], (params, p)
        unreal += int((~real).sum())
    assert unreal > 0


def test_the_fixture_is_what_the_restatement_gives(small):
    fx, sel, _, _, traced = small
    gold = align_trace_util.Fixture()
    assert gold.runs.shape == fx.result.shape[:2] and gold.sha256.shape == fx.result.shape[:2] + (32,) and gold.real.shape == gold.runs.shape
    assert os.path.getsize(align_trace_util.FIXTURE) < 64 * 1024
    assert (gold.runs >= 1).all()
    for s in range(len(fx.params)):
        _, ops, real = traced[s]
        assert [len(o) for o in ops] == gold.runs[s][sel].tolist()
        assert [align_trace_util.digest(o) for o in ops] == [gold.sha256[s][p].tobytes() for p in sel]
        assert np.array_equal(real, gold.real[s][sel])


def test_the_kernels_schedule_stores_and_walks_under_sanitizers(tmp_path, small):
    fx, sel, firsts, seconds, traced = small
    exe = tmp_path / "align_trace_schedule_check"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        "-I", os.path.join(ROOT, "meshclust2_amd", "csrc"), os.path.join(ROOT, "tests", "align_trace_schedule_check.cpp"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    # the edges under five parameter sets (two of them with paths that are not real), then the small fixture pairs under the fixture's three
    ea, eb = align_trace_util.edge_pairs()
    sets = np.array([[1, -1, 2, 1], [2, -3, 5, 2], [1, -1, 0, 1], [1, 1, 0, 0], [0, 0, 1, 1]])
    edge_ops = [align_trace_util.trace_many(ea, eb, params)[1] for params in sets]
    dumps = [(tmp_path / "edges.txt", ea + eb, sets, np.arange(len(ea)), np.arange(len(ea)) + len(ea), edge_ops),
             (tmp_path / "small.txt", firsts + seconds, fx.params, np.arange(sel.size), np.arange(sel.size) + sel.size, [t[1] for t in traced])]
    runs = []
    for path, seqs, params, first, second, ops in dumps:
        align_trace_util.write_dump(str(path), seqs, params, first, second, ops)
        runs.append((subprocess.Popen([str(exe), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT), len(first), len(params)))
    for run, n_pairs, n_sets in runs:
        out = run.communicate(timeout=600)[0]
        assert run.returncode == 0 and b"%d pairs under %d parameter sets agree" % (n_pairs, n_sets) in out, out.decode()[-2000:]
    # the program does fail on a difference: one run of one pair a column longer
    wrong = [[o.copy() for o in per_set] for per_set in edge_ops[:2]]
    wrong[1][6][0] += 16
    path = tmp_path / "wrong.txt"
    align_trace_util.write_dump(str(path), ea + eb, sets[:2], np.arange(8), np.arange(8) + len(ea), [w[:8] for w in wrong])
    r = subprocess.run([str(exe), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 1 and b"set 1 pair 6" in r.stdout, r.stdout.decode()[-2000:]
