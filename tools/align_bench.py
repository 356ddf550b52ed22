#!/usr/bin/env python3
"""msc_align_pairs on synthetic pairs -- run on the GPU box.

    python tools/align_bench.py [--reps 3]

Three shapes, built here from meshclust2_amd/synth.py (members of one family against each other: 3 % substitutions, 0.5 % indels):
1 000 pairs of 1 kb, 20 000 pairs of 1 kb and 200 pairs of 20 kb. One JSON line per shape: pairs, cells (the sum of la * lb), the best wall
time of `reps` calls after a warm-up call (a call uploads the sequences, runs the kernel and brings the integers back), cells per second,
and the kernel msc_last_kernel_info named. A last line repeats the cells per second beside the issue rate of the chip's vector units for
the instruction count given with --valu-per-cell (counted in the cell loop's ISA; profiles/align.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshclust2_amd import api, synth          # noqa: E402

SHAPES = [("1000 x 1 kb", 1000, 1000), ("20000 x 1 kb", 20000, 1000), ("200 x 20 kb", 200, 20000)]


def pairs_of(n_pairs, length, seed):
    n_seqs = min(2 * n_pairs, 2000 if length <= 1000 else 80)
    seqs, _ = synth.families(seed, n_seqs, length, family=20)
    first = np.arange(n_pairs, dtype=np.uint32) % n_seqs
    second = (first // 20) * 20 + (first % 20 + 1 + (np.arange(n_pairs) // n_seqs) % 18) % 20          # another member of the same family
    return seqs, first, np.minimum(second, n_seqs - 1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--valu-per-cell", type=float, default=0.0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    ctx = api.Context(args.device)
    rates = {}
    for name, n_pairs, length in SHAPES:
        seqs, first, second = pairs_of(n_pairs, length, 77 + length)
        ln = np.array([len(s) for s in seqs], dtype=np.int64)
        cells = int((ln[first] * ln[second]).sum())
        api.align_pairs(ctx, seqs, first, second)          # warm-up: scratch buffers, code object
        best = None
        for _ in range(args.reps):
            t = time.perf_counter()
            r = api.align_pairs(ctx, seqs, first, second)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        rates[name] = cells / best
        print(json.dumps({"shape": name, "pairs": n_pairs, "cells": cells, "seconds": round(best, 6), "cells_per_s": round(cells / best), "kernel": ctx.last_kernel_info()[0],
                          "mean_identity": round(float(r["identity"].mean()), 4)}), flush=True)
    if args.valu_per_cell > 0:
        # 256 CUs x 4 SIMDs, one wave64 VALU instruction per SIMD every 4 cycles = 64 lanes' cells per instruction, 2.4 GHz
        issue = 256 * 4 * 64 / 4 * 2.4e9
        print(json.dumps({"valu_per_cell": args.valu_per_cell, "issue_bound_cells_per_s": round(issue / args.valu_per_cell),
                          "fraction_of_issue_rate": {k: round(v * args.valu_per_cell / issue, 4) for k, v in rates.items()}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
