#!/usr/bin/env python3
"""Writes tests/golden/align_pairs.npz: sequences, a pair list, three parameter sets and the (score, length, matches) the REFERENCE's own
global aligner gives for every pair under every set.

    python tests/golden/gen_align_golden.py --reference /path/to/MeShClust2

The sequences are seeded (meshclust2_amd/synth.py). The results come from a small program, written here, that is compiled in a scratch
directory against the reference's utility/GlobAlignE.cpp and calls its constructor the way Feature::align does (predict/Feature.cpp:697-718),
with the parameters of the set. The class hands out its score, its length and the quotient matches / length; the program prints the
integers (matches = the quotient times the length, rounded: exact, both are below 2^16). Nothing of the reference is copied into the repository."""
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

from align_util import write_dump          # noqa: E402
from meshclust2_amd import synth           # noqa: E402

PARAMS = [(1, -1, 2, 1), (2, -3, 5, 2), (1, -1, 0, 1)]
EDGE_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257]

HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>
#include "GlobAlignE.h"
int main() {
	size_t n_seqs, n_sets, n_pairs;
	std::cin >> n_seqs >> n_sets >> n_pairs;
	std::vector<std::string> seqs(n_seqs);
	for (auto& s : seqs) std::cin >> s;
	std::vector<int> par(4 * n_sets);
	for (auto& v : par) std::cin >> v;
	std::vector<unsigned> pr(2 * n_pairs);
	for (auto& v : pr) std::cin >> v;
	for (size_t s = 0; s < n_sets; s++)
		for (size_t p = 0; p < n_pairs; p++) {
			const std::string &a = seqs[pr[2 * p]], &b = seqs[pr[2 * p + 1]];
			utility::GlobAlignE g(a.c_str(), 0, (int)a.size() - 1, b.c_str(), 0, (int)b.size() - 1, par[4 * s], par[4 * s + 1], par[4 * s + 2], par[4 * s + 3]);
			const int len = g.getLength();
			printf("%d %d %ld\n", g.getScore(), len, std::lround(g.getIdentity() * len));
		}
	return 0;
}
"""


def build_cases():
    seqs, pairs = [], []

    def add(s):
        seqs.append(bytes(s))
        return len(seqs) - 1

    def both(a, b):
        pairs.append((a, b))
        if seqs[a] != seqs[b]:
            pairs.append((b, a))

    # the edge lengths: prefixes of the members of one family (related, with indels), against each other, themselves and a member of 300
    fam, _ = synth.families(7, len(EDGE_LENGTHS) + 1, 330, family=len(EDGE_LENGTHS) + 1)
    edge = [add(fam[k][:n]) for k, n in enumerate(EDGE_LENGTHS)]
    s300 = add(fam[-1][:300])
    for a in edge:
        for b in edge:
            pairs.append((a, b))          # (both orders and a == b: a sequence against itself)
        both(a, s300)
    pairs.append((s300, s300))
    # (1, 1) equal and unequal
    a1, a2, c1 = add(b"A"), add(b"A"), add(b"C")
    pairs.append((a1, a2))
    both(a1, c1)
    # no identical column at all; homopolymers and (AC)n against shifted copies of themselves: every tie rule fires
    all_a, all_c, short_c = add(b"A" * 100), add(b"C" * 100), add(b"C" * 37)
    both(all_a, all_c)
    both(all_a, short_c)
    both(all_a, add(b"A" * 97))
    both(all_a, add(b"A" * 260))
    ac = add(b"AC" * 70)
    both(ac, add((b"AC" * 70)[1:]))
    both(ac, add((b"AC" * 70)[3:] + b"A"))
    both(ac, add(b"CA" * 70))
    both(ac, add(b"AC" * 131))
    pairs.append((ac, ac))
    # the corner where the stand-in for minus infinity wins: 40 against 3 000
    long3k = synth.to_ascii(synth.template(21, 0, 3000))
    l3k = add(long3k)
    both(add(long3k[1480:1520]), l3k)
    both(add(synth.to_ascii(synth.template(21, 1, 40))), l3k)
    # runs of N
    base = bytearray(fam[3][:300])
    n1, n2 = bytearray(base), bytearray(fam[4][:290])
    n1[20:55] = b"N" * 35
    n2[40:48] = b"N" * 8
    n2[200:290] = b"N" * 90
    i1, i2 = add(n1), add(n2)
    both(i1, i2)
    both(i1, add(base))
    pairs.append((i2, i2))
    both(add(b"N" * 70), i2)
    # mutated 1 kb families (3 % substitutions, 0.5 % indels)
    kb, _ = synth.families(11, 5, 1000, family=5, sub_rate=0.03, indel_rate=0.005)
    kbi = [add(s) for s in kb]
    for a in kbi:
        for b in kbi:
            if a != b:
                pairs.append((a, b))
    # 1 500 x 2 000, 8 000 x 8 000 and 32 767 x 300
    t2k = synth.template(31, 0, 2000)
    both(add(synth.to_ascii(synth.member(31, 0, 0, t2k))[:1500]), add(synth.to_ascii(t2k)))
    t8k = synth.template(33, 0, 8000)
    m8k = synth.to_ascii(synth.member(33, 0, 0, t8k))
    m8k = (m8k + synth.to_ascii(t8k))[:8000]
    both(add(m8k), add(synth.to_ascii(t8k)))
    longest = bytearray(synth.to_ascii(synth.template(35, 0, 32767)))
    longest[20000:20300] = fam[-1][:300]          # (the short one occurs inside the long one)
    both(add(longest), s300)
    return seqs, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (its src/utility/GlobAlignE.cpp is compiled)")
    ap.add_argument("--out", default=os.path.join(HERE, "align_pairs.npz"))
    args = ap.parse_args()
    seqs, pairs = build_cases()
    first = np.array([p[0] for p in pairs], dtype=np.uint32)
    second = np.array([p[1] for p in pairs], dtype=np.uint32)
    util = os.path.join(args.reference, "src", "utility")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, dump = os.path.join(tmp, "harness.cpp"), os.path.join(tmp, "harness"), os.path.join(tmp, "pairs.txt")
        open(src, "w").write(HARNESS)
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-w", "-I", util, src, os.path.join(util, "GlobAlignE.cpp"), "-o", exe])
        write_dump(dump, seqs, PARAMS, first, second)
        text = subprocess.check_output([exe], stdin=open(dump))
    result = np.array(text.split(), dtype=np.int32).reshape(len(PARAMS), len(pairs), 3)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    np.savez_compressed(args.out, text=np.frombuffer(b"".join(seqs), dtype=np.uint8), offsets=offsets, first=first, second=second,
                        params=np.array(PARAMS, dtype=np.int32), result=result)
    print("%d sequences, %d pairs, %d parameter sets -> %s (%d bytes)" % (len(seqs), len(pairs), len(PARAMS), args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
