#!/usr/bin/env python3
"""Writes tests/golden/align_long.npz: pairs with a sequence past 32 767 bytes, and the (score, length, matches) the REFERENCE's own global
aligner gives for them -- the fixture of msc_align_pairs_long.

    python tests/golden/gen_align_long_golden.py --reference /path/to/MeShClust2

The method is gen_align_golden.py's: the sequences are seeded (meshclust2_amd/synth.py), the results come from that file's small program,
compiled in a scratch directory against the reference's utility/GlobAlignE.cpp (matches = the quotient times the length, rounded: exact in
a double, both are below 2^22). Nothing of the reference is copied into the repository. The thin and the unrelated pairs run under the three
parameter sets of align_pairs.npz, the large grids under the default set only (`have` says which); the whole list takes a few minutes.

Two properties the tests rely on are asserted HERE, on the reference's integers: the last two pairs have more than 65 535 identical
columns, and the 99 % pair's score satisfies the certificate of 4.6f at half-width 1 024."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import align_band_util                              # noqa: E402
from align_util import write_dump                   # noqa: E402
from gen_align_golden import HARNESS, PARAMS        # noqa: E402
from meshclust2_amd import synth                    # noqa: E402

CERTIFIED_AT = 1024


def build_cases():
    """-> seqs, pairs, every[p] (True: all three parameter sets, False: the default set only), names of the pairs the tests look up"""
    seqs, pairs, every, names = [], [], [], {}

    def add(s):
        seqs.append(bytes(s))
        return len(seqs) - 1

    def both(a, b, all_sets):
        pairs.extend([(a, b), (b, a)])
        every.extend([all_sets, all_sets])

    short = synth.to_ascii(synth.template(41, 0, 300))
    s300 = add(short)
    for seed, n in ((43, 32768), (45, 70000)):          # the first length past the old limit; the first whose length << 16 no longer fits
        long_one = bytearray(synth.to_ascii(synth.template(seed, 0, n)))
        long_one[n - 9000:n - 8700] = short              # (the short one occurs inside the long one)
        both(add(long_one), s300, True)
    # unrelated, 40 000 x 5 000: the stand-in for minus infinity at size
    names["unrelated"] = len(pairs)
    both(add(synth.to_ascii(synth.template(47, 0, 40000))), add(synth.to_ascii(synth.template(47, 1, 5000))), True)
    # related at the default rates, 40 000 x about 33 000: a full grid of many tiles
    t40k = synth.template(49, 0, 40000)
    names["many_tiles"] = len(pairs)
    both(add(synth.to_ascii(t40k)), add(synth.to_ascii(synth.member(49, 0, 0, t40k[3000:36000]))), False)
    # 70 000 x about 70 000 at 99 %: more identical columns than 16 bits count
    t70k = synth.template(51, 0, 70000)
    names["similar"] = len(pairs)
    pairs.append((add(synth.to_ascii(t70k)), add(synth.to_ascii(synth.member(51, 0, 0, t70k, sub_rate=0.008, indel_rate=0.002)))))
    every.append(False)
    # homopolymers: every tie rule, with wide counts
    names["homopolymer"] = len(pairs)
    pairs.append((add(b"A" * 66000), add(b"A" * 65600)))
    every.append(False)
    return seqs, pairs, np.array(every), names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (its src/utility/GlobAlignE.cpp is compiled)")
    ap.add_argument("--out", default=os.path.join(HERE, "align_long.npz"))
    args = ap.parse_args()
    seqs, pairs, every, names = build_cases()
    first = np.array([p[0] for p in pairs], dtype=np.uint32)
    second = np.array([p[1] for p in pairs], dtype=np.uint32)
    util = os.path.join(args.reference, "src", "utility")
    result = np.zeros((len(PARAMS), len(pairs), 3), dtype=np.int32)
    have = np.zeros((len(PARAMS), len(pairs)), dtype=bool)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "harness.cpp"), os.path.join(tmp, "harness")
        open(src, "w").write(HARNESS)
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-w", "-I", util, src, os.path.join(util, "GlobAlignE.cpp"), "-o", exe])
        runs = []          # a run per group of pairs and parameter set, side by side
        for s in range(len(PARAMS)):
            sel = np.nonzero(every if s else np.ones_like(every))[0]
            for part in (sel[every[sel]], sel[~every[sel]][:2], sel[~every[sel]][2:3], sel[~every[sel]][3:]):
                if part.size == 0:
                    continue
                dump = os.path.join(tmp, "pairs%d_%d.txt" % (s, len(runs)))
                write_dump(dump, seqs, PARAMS[s:s + 1], first[part], second[part])
                runs.append((s, part, subprocess.Popen([exe], stdin=open(dump), stdout=subprocess.PIPE)))
        for s, part, run in runs:
            text = run.communicate()[0]
            assert run.returncode == 0
            result[s, part] = np.array(text.split(), dtype=np.int32).reshape(part.size, 3)
            have[s, part] = True
    ln = np.array([len(s) for s in seqs], dtype=np.int64)
    for key in ("similar", "homopolymer"):
        p = names[key]
        assert result[0, p, 2] > 65535, (key, result[0, p].tolist())
    p = names["similar"]
    assert align_band_util.certified(int(ln[first[p]]), int(ln[second[p]]), CERTIFIED_AT, PARAMS[0], int(result[0, p, 0])), result[0, p].tolist()
    offsets = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    np.savez_compressed(args.out, text=np.frombuffer(b"".join(seqs), dtype=np.uint8), offsets=offsets, first=first, second=second,
                        params=np.array(PARAMS, dtype=np.int32), result=result, have=have,
                        names=np.array(sorted(names)), named=np.array([names[k] for k in sorted(names)], dtype=np.int64))
    for s in range(len(PARAMS)):
        for p in np.nonzero(have[s])[0]:
            print("set %d pair %2d  %6d x %6d  ->  %s" % (s, p, ln[first[p]], ln[second[p]], result[s, p].tolist()))
    print("%d sequences, %d pairs -> %s (%d bytes)" % (len(seqs), len(pairs), args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
