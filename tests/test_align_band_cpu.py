"""msc_align_pairs_banded / msc_align_pairs_auto without a device. (1) tests/align_band_util.py, the numpy restatement of the
banded operator and its certificate, equals the unbanded restatement (tests/align_util.py, which tests/test_align_cpu.py holds to the
reference's own integers) once the band covers the grid. (2) The certificate is sound: over every pair of a two-letter alphabet up to 5 x 5,
half-widths 0 .. 4 and 19 parameter sets, no certified triple differs from the full one, and without an offer only a covering band certifies.
(3) tests/align_band_schedule_check.cpp replays the kernel's schedule serially over csrc/msc_align_band.h -- the code the kernel compiles --
on every fixture pair at eight half-widths, under each number of columns per lane, in a stand-alone program built with the address and
undefined-behaviour sanitizers, against a dump the restatement wrote."""
import itertools
import os
import subprocess

import numpy as np

import align_band_util
import align_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = [0, 1, 7, 63, 64, 255, 256, 300]


def test_a_band_that_covers_the_grid_is_the_full_alignment():
    fx = align_util.Fixture()
    sel = np.nonzero(fx.cells() <= 300 * 300)[0]
    assert sel.size > 150
    firsts, seconds = [fx.seqs[i] for i in fx.first[sel]], [fx.seqs[i] for i in fx.second[sel]]
    mn = np.array([min(len(a), len(b)) for a, b in zip(firsts, seconds)])
    for s, params in enumerate(fx.params):
        want = align_util.align_many(firsts, seconds, params)
        assert np.array_equal(want, fx.result[s][sel])
        for bands in (mn, mn + 3, 40000, 0xffffffff):          # w = min(la, lb) is the smallest that covers
            got = align_band_util.banded_many(firsts, seconds, bands, params)
            bad = np.nonzero((got[:, :3] != want).any(axis=1))[0]
            assert bad.size == 0, (params.tolist(), sel[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
            assert got[:, 3].all()
    # one pair at a time gives what the batch gives; the narrowest band changes some pairs' triples, and those are not certified
    got = align_band_util.banded_many(firsts, seconds, 0, fx.params[0])
    assert list(align_band_util.banded(firsts[44], seconds[44], 0, fx.params[0])) == got[44].tolist()
    differs = (got[:, :3] != fx.result[0][sel]).any(axis=1)
    assert differs.any() and not got[differs, 3].any()


def test_no_certified_triple_differs_from_the_full_one():
    seqs = [bytes(x) for n in range(1, 6) for x in itertools.product(b"AC", repeat=n)]
    firsts = [a for a in seqs for _ in seqs]
    seconds = [b for _ in seqs for b in seqs]
    mn = np.array([min(len(a), len(b)) for a, b in zip(firsts, seconds)])
    assert len(seqs) == 62 and len(align_band_util.OFFERED) == 16 and len(align_band_util.REFUSED) == 3
    cases = certified = 0
    for params in align_band_util.OFFERED + align_band_util.REFUSED:
        assert align_band_util.offered(params) == (params in align_band_util.OFFERED)
        full = align_util.align_many(firsts, seconds, params, step=8)
        for w in range(5):
            got = align_band_util.banded_many(firsts, seconds, w, params, step=8)
            flag = got[:, 3] == 1
            bad = np.nonzero(flag & (got[:, :3] != full).any(axis=1))[0]
            assert bad.size == 0, (params, w, firsts[bad[0]], seconds[bad[0]], got[bad[0]].tolist(), full[bad[0]].tolist())
            assert flag[w >= mn].all()
            if params in align_band_util.REFUSED:
                assert not flag[w < mn].any()
            cases += flag.size
            certified += int(flag.sum())
    assert cases == 19 * 5 * 62 * 62 and certified > cases // 2, (cases, certified)          # (a certificate that never says yes passes nothing here)
    # the conditions of the offer are needed: with gap_open < 0 a narrow band does change a triple
    params = align_band_util.REFUSED[0]
    assert (align_band_util.banded_many(firsts, seconds, 0, params, step=8)[:, :3] != align_util.align_many(firsts, seconds, params, step=8)).any()


def test_the_kernels_schedule_on_every_fixture_pair_under_sanitizers(tmp_path):
    fx = align_util.Fixture()
    exe = tmp_path / "align_band_schedule_check"
    build = subprocess.Popen(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                              "-I", os.path.join(ROOT, "meshclust2_amd", "csrc"), os.path.join(ROOT, "tests", "align_band_schedule_check.cpp"), "-o", str(exe)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    n = fx.first.size
    firsts, seconds = [fx.seqs[i] for i in fx.first] * len(BANDS), [fx.seqs[i] for i in fx.second] * len(BANDS)
    bands = np.repeat(BANDS, n)
    want = np.zeros((len(fx.params), len(BANDS), n, 4), dtype=np.int64)
    for s, params in enumerate(fx.params):          # (a pair's eight half-widths share a batch: the long pairs cost one walk over their diagonals)
        want[s] = align_band_util.banded_many(firsts, seconds, bands, params).reshape(len(BANDS), n, 4)
        certified = want[s][:, :, 3] == 1
        assert (want[s][:, :, :3][certified] == np.broadcast_to(fx.result[s], (len(BANDS), n, 3))[certified]).all()
    assert build.wait(timeout=300) == 0, build.stdout.read().decode()
    runs = []          # a run per parameter set, side by side
    for s in range(len(fx.params)):
        dump = tmp_path / ("pairs%d.txt" % s)
        align_band_util.write_dump(str(dump), fx.seqs, fx.params[s:s + 1], fx.first, fx.second, BANDS, want[s:s + 1])
        runs.append(subprocess.Popen([str(exe), str(dump)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for s, run in enumerate(runs):
        out = run.communicate(timeout=900)[0]
        assert run.returncode == 0 and b"%d pairs at 8 half-widths under 1 parameter sets agree, %d certified" % (n, int(want[s][:, :, 3].sum())) in out, (s, out.decode()[-2000:])
    # the program does fail on a difference: one flag turned in the dump
    wrong = want[:, :, :8].copy()
    wrong[2, 3, 7, 3] ^= 1
    dump = tmp_path / "pairs.txt"
    align_band_util.write_dump(str(dump), fx.seqs, fx.params, fx.first[:8], fx.second[:8], BANDS, wrong)
    r = subprocess.run([str(exe), str(dump)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 1 and b"set 2 band 63 pair 7" in r.stdout, r.stdout.decode()[-2000:]
