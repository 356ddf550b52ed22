"""msc_align_pairs without a device. (1) tests/align_util.py, the numpy restatement of the recurrence the GPU tests lean on, is held to the
reference's own results (tests/golden/align_pairs.npz, written by tests/golden/gen_align_golden.py from the reference's GlobAlignE) on every
fixture pair of at most 300 x 300 cells, under each of the three parameter sets, exactly. (2) tests/align_schedule_check.cpp replays the
kernel's schedule serially over csrc/msc_align.h -- the cell update the kernel compiles -- on EVERY fixture pair (the 8 000 x 8 000 and
32 767 x 300 ones included) in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np

import align_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_fixture_holds_the_cases():
    fx = align_util.Fixture()
    ln = np.array([len(s) for s in fx.seqs])
    shapes = set(zip(ln[fx.first].tolist(), ln[fx.second].tolist()))
    edge = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    for a in edge:
        for b in edge:
            assert (a, b) in shapes
        assert (a, 300) in shapes and (300, a) in shapes
    for shape in ((40, 3000), (3000, 40), (1500, 2000), (2000, 1500), (8000, 8000), (32767, 300), (300, 32767)):
        assert shape in shapes, shape
    assert fx.params.tolist() == [[1, -1, 2, 1], [2, -3, 5, 2], [1, -1, 0, 1]]
    assert fx.result.shape == (3, fx.first.size, 3)
    listed = set(zip(fx.first.tolist(), fx.second.tolist()))
    for a, b in listed:          # both argument orders of every unequal pair
        assert fx.seqs[a] == fx.seqs[b] or (b, a) in listed
    assert any(a == b for a, b in listed) and any(b"N" * 30 in s for s in fx.seqs)
    assert os.path.getsize(align_util.FIXTURE) < 256 * 1024


def test_the_restatement_is_the_reference_on_the_small_pairs():
    fx = align_util.Fixture()
    sel = np.nonzero(fx.cells() <= 300 * 300)[0]
    assert sel.size > 150
    firsts, seconds = [fx.seqs[i] for i in fx.first[sel]], [fx.seqs[i] for i in fx.second[sel]]
    for s, params in enumerate(fx.params):
        got = align_util.align_many(firsts, seconds, params)
        bad = np.nonzero((got != fx.result[s][sel]).any(axis=1))[0]
        assert bad.size == 0, (params.tolist(), sel[bad[0]], got[bad[0]].tolist(), fx.result[s][sel[bad[0]]].tolist())
    # one pair at a time gives what the batch gives, and the order of the arguments matters
    one = align_util.align(firsts[5], seconds[5], fx.params[1])
    assert list(one) == align_util.align_many(firsts, seconds, fx.params[1])[5].tolist()
    assert (fx.result[0][:, 1] > 0).all() and (fx.result[:, :, 2] <= fx.result[:, :, 1]).all()


def test_the_kernels_schedule_on_every_fixture_pair_under_sanitizers(tmp_path):
    fx = align_util.Fixture()
    exe = tmp_path / "align_schedule_check"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        "-I", os.path.join(ROOT, "meshclust2_amd", "csrc"), os.path.join(ROOT, "tests", "align_schedule_check.cpp"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    runs = []          # a run per parameter set, side by side
    for s in range(len(fx.params)):
        dump = tmp_path / ("pairs%d.txt" % s)
        align_util.write_dump(str(dump), fx.seqs, fx.params[s:s + 1], fx.first, fx.second, fx.result[s:s + 1])
        runs.append(subprocess.Popen([str(exe), str(dump)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for s, run in enumerate(runs):
        out = run.communicate(timeout=600)[0]
        assert run.returncode == 0 and b"%d pairs under 1 parameter sets agree" % fx.first.size in out, (s, out.decode()[-2000:])
    dump = tmp_path / "pairs.txt"
    # the program does fail on a difference: one wrong count in the dump
    wrong = fx.result.copy()
    wrong[2, 7, 2] += 1
    align_util.write_dump(str(dump), fx.seqs, fx.params, fx.first[:8], fx.second[:8], wrong[:, :8])
    r = subprocess.run([str(exe), str(dump)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 1 and b"set 2 pair 7" in r.stdout, r.stdout.decode()[-2000:]
