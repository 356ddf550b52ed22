"""msc_align_pairs_long without a device: tests/align_long_schedule_check.cpp replays the schedule of k_align_tiles in launch
order over csrc/msc_align_long.h, csrc/msc_align_band.h and csrc/msc_align.h -- the code the kernel compiles -- with the borders in one host
array per pair laid out as on the device, poisoned, and every entry stamped with the launch that wrote it. (1) Built with the address and
undefined-behaviour sanitizers it runs every pair of tests/golden/align_pairs.npz of at most 9 000 000 cells under the fixture's three
parameter sets, at 64, 100 and 1 024 rows a tile, over the full grid and at half-widths 1, 64 and 300, against a plain loop nest over the
rows (uncertified triples too) and against the reference's integers. (2) Built plainly it runs the thin pairs of tests/golden/align_long.npz
over the full grid, and the 70 000 x 70 000 pair at half-width 1 024, which must come out certified and equal to the reference's integers."""
import os
import subprocess

import numpy as np

import align_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = os.path.join(ROOT, "tests", "golden", "align_long.npz")
SOURCE = os.path.join(ROOT, "tests", "align_long_schedule_check.cpp")
FLAGS = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "meshclust2_amd", "csrc"), SOURCE]


def test_the_tile_schedule_on_the_short_fixture_under_sanitizers(tmp_path):
    fx = align_util.Fixture()
    exe = tmp_path / "align_long_schedule_check"
    r = subprocess.run(FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    sel = np.nonzero(fx.cells() <= 9000000)[0]
    assert sel.size >= 190
    runs = []          # a run per parameter set, side by side
    for s in range(len(fx.params)):
        dump = tmp_path / ("pairs%d.txt" % s)
        align_util.write_dump(str(dump), fx.seqs, fx.params[s:s + 1], fx.first[sel], fx.second[sel], fx.result[s:s + 1, sel])
        runs.append(subprocess.Popen([str(exe), str(dump), "--rows", "64,100,1024", "--bands", "full,1,64,300", "--nest"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for s, run in enumerate(runs):
        out = run.communicate(timeout=1500)[0]
        assert run.returncode == 0 and b"%d pairs under 1 parameter sets: %d runs agree" % (sel.size, sel.size * 12) in out, (s, out.decode()[-2000:])
    # the program does fail on a difference: one count turned in the dump
    wrong = fx.result[:, sel[:8]].copy()
    wrong[1, 5, 2] += 1
    dump = tmp_path / "pairs.txt"
    align_util.write_dump(str(dump), fx.seqs, fx.params, fx.first[sel[:8]], fx.second[sel[:8]], wrong)
    r = subprocess.run([str(exe), str(dump), "--rows", "64", "--bands", "full"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 1 and b"set 1 pair 5" in r.stdout and b"the dump holds" in r.stdout, r.stdout.decode()[-2000:]


def test_the_tile_schedule_on_the_long_fixture(tmp_path):
    fx = align_util.Fixture(LONG)
    z = np.load(LONG)
    have, named = z["have"], dict(zip(z["names"].tolist(), z["named"].tolist()))
    ln = np.array([len(s) for s in fx.seqs])
    exe = tmp_path / "align_long_schedule_check"
    r = subprocess.run(FLAGS + ["-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    thin = np.nonzero(np.minimum(ln[fx.first], ln[fx.second]) <= 300)[0]
    assert thin.size == 4 and have[:, thin].all() and ln[fx.first[thin]].max() == 70000
    dump = tmp_path / "thin.txt"
    align_util.write_dump(str(dump), fx.seqs, fx.params, fx.first[thin], fx.second[thin], fx.result[:, thin])
    full = subprocess.Popen([str(exe), str(dump), "--rows", "1024", "--bands", "full"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    p = named["similar"]
    assert ln[fx.first[p]] == 70000 and fx.result[0, p, 2] > 65535          # more identical columns than 16 bits count
    dump = tmp_path / "similar.txt"
    align_util.write_dump(str(dump), fx.seqs, fx.params[:1], fx.first[p:p + 1], fx.second[p:p + 1], fx.result[:1, p:p + 1])
    banded = subprocess.Popen([str(exe), str(dump), "--rows", "1024", "--bands", "1024", "--must-certify"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = full.communicate(timeout=900)[0]
    assert full.returncode == 0 and b"4 pairs under 3 parameter sets: 12 runs agree, 12 certified" in out, out.decode()[-2000:]
    out = banded.communicate(timeout=900)[0]
    assert banded.returncode == 0 and b"1 pairs under 1 parameter sets: 1 runs agree, 1 certified" in out, out.decode()[-2000:]
