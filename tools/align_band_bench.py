#!/usr/bin/env python3
"""msc_align_pairs_banded and msc_align_pairs_auto against msc_align_pairs on the same pairs in the same process -- run on the GPU box.

    python tools/align_band_bench.py [--reps 3] [--shapes 0,1,2,3,4] [--first-band 0] [--distinct 0]

Shapes: 20 000 pairs of 1 kb at 97 % and at 90 % identity, 1 000 pairs of 5 kb at 95 %, 200 pairs of 20 kb at 95 % and at 85 %. A pair is a random
ACGT template and a mutant of it by msc_cluster.cpp's recipe (rate = 1 - identity: 0.8 of it substitutions, 0.1 deletions, 0.1 insertions).
--distinct N lists each of N (template, mutant) pairs n_pairs / N times, so that the upload of the text (40 MB for 20 000 distinct pairs of
1 kb, which costs more than their kernels) shrinks and the kernels' share of the time shows.
Per shape: the smallest power-of-two half-width at which msc_align_pairs_banded certifies every pair is searched first (untimed); then `reps`
rounds of (msc_align_pairs, msc_align_pairs_banded at that band, msc_align_pairs_auto), alternating, after one warm-up round; the medians of
the wall times (a call uploads the sequences, runs its kernels and brings the integers back). One JSON line per shape and call with the cells
the call filled (window rows x stripe columns, summed over stripes and, for auto, over rounds), the cells inside the band, the cells of the
full grid, cells filled per second, the columns-per-lane variants the pairs took and, for auto, the pairs per round. Every triple is compared
with msc_align_pairs's before a time is reported."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshclust2_amd import api          # noqa: E402

SHAPES = [("20000 x 1 kb, 97 %", 20000, 1000, 0.03), ("20000 x 1 kb, 90 %", 20000, 1000, 0.10), ("1000 x 5 kb, 95 %", 1000, 5000, 0.05),
          ("200 x 20 kb, 95 %", 200, 20000, 0.05), ("200 x 20 kb, 85 %", 200, 20000, 0.15)]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NO_BAND = 0xffffffff


def mutant(rs, codes, rate):
    u = rs.rand(codes.size)
    sub = u < rate * 0.8
    out = codes.copy()
    out[sub] = ACGT[rs.randint(0, 4, int(sub.sum()))]
    copies = np.where((u >= rate * 0.8) & (u < rate * 0.9), 0, np.where((u >= rate * 0.9) & (u < rate), 2, 1))
    out = np.repeat(out, copies)
    inserted = np.nonzero(np.repeat(copies == 2, copies))[0][1::2]
    out[inserted] = ACGT[rs.randint(0, 4, inserted.size)]
    return out.tobytes()


# the schedule's sizes, as csrc/msc_align_band.h has them
def diagonals(la, lb, w):
    return abs(la - lb) + 2 * w + 1


def cols_of(la, lb, w):
    d = diagonals(la, lb, w)
    return 1 if d <= 128 else 2 if d <= 512 else 4


def worth(la, lb, w):
    return w < min(la, lb) and 2 * min(lb, diagonals(la, lb, w) + 64 * cols_of(la, lb, w) - 1) <= lb


def cells_filled(la, lb, w):
    stripe = 64 * cols_of(la, lb, w)
    lo, hi = min(0, la - lb) - w, max(0, la - lb) + w
    c0 = np.arange(1, la + 1, stripe)
    c1 = np.minimum(c0 + stripe - 1, la)
    rows = np.minimum(lb, c1 - lo) - np.maximum(1, c0 - hi) + 1
    return int(rows.sum()) * stripe


def cells_in_band(la, lb, w):
    lo, hi = min(0, la - lb) - w, max(0, la - lb) + w
    j = np.arange(1, lb + 1)
    return int((np.minimum(la, j + hi) - np.maximum(1, j + lo) + 1).clip(0).sum())


def full_filled(la, lb):
    return -(-la // 256) * 256 * lb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2,3,4")
    ap.add_argument("--first-band", type=int, default=0)
    ap.add_argument("--distinct", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    ctx = api.Context(args.device)
    for at in [int(v) for v in args.shapes.split(",")]:
        name, n_pairs, length, rate = SHAPES[at]
        rs = np.random.RandomState(500 + at)
        seqs = []
        distinct = min(n_pairs, args.distinct) if args.distinct else n_pairs
        for _ in range(distinct):
            t = ACGT[rs.randint(0, 4, length)]
            seqs.extend((t.tobytes(), mutant(rs, t, rate)))
        first = (2 * (np.arange(n_pairs) % distinct)).astype(np.uint32)
        second = first + 1
        la = np.array([len(seqs[i]) for i in first])
        lb = np.array([len(seqs[i]) for i in second])
        full = api.align_pairs(ctx, seqs, first, second)          # (warm-up of the baseline too)
        band = 1
        while True:          # the smallest power of two that certifies every pair
            r = api.align_pairs_banded(ctx, seqs, first, second, band)
            if r["certified"].all():
                break
            band *= 2
        auto = api.align_pairs_auto(ctx, seqs, first, second, first_band=args.first_band)
        for got in (r, auto):
            assert all(np.array_equal(got[k], full[k]) for k in ("score", "length", "matches")), name
        times = {"full": [], "banded": [], "auto": []}
        for _ in range(args.reps):
            for what, call in (("full", lambda: api.align_pairs(ctx, seqs, first, second)), ("banded", lambda: api.align_pairs_banded(ctx, seqs, first, second, band)),
                               ("auto", lambda: api.align_pairs_auto(ctx, seqs, first, second, first_band=args.first_band))):
                t = time.perf_counter()
                call()
                times[what].append(time.perf_counter() - t)
        grid = int((la * lb).sum())
        med = {k: statistics.median(v) for k, v in times.items()}
        filled = sum(full_filled(int(a), int(b)) for a, b in zip(la, lb))
        print(json.dumps({"shape": name, "call": "msc_align_pairs", "seconds": round(med["full"], 6), "cells_filled": filled, "cells_grid": grid,
                          "cells_filled_per_s": round(filled / med["full"]), "mean_identity": round(float(full["identity"].mean()), 4)}), flush=True)
        filled = sum(cells_filled(int(a), int(b), band) for a, b in zip(la, lb))
        variants = sorted(set(cols_of(int(a), int(b), band) for a, b in zip(la, lb)))
        print(json.dumps({"shape": name, "call": "msc_align_pairs_banded", "band": band, "seconds": round(med["banded"], 6), "speedup": round(med["full"] / med["banded"], 3),
                          "cells_filled": filled, "cells_in_band": sum(cells_in_band(int(a), int(b), band) for a, b in zip(la, lb)), "cells_grid": grid,
                          "cells_filled_per_s": round(filled / med["banded"]), "columns_per_lane": variants}), flush=True)
        w0 = args.first_band or 64
        rounds, filled, in_band, variants, to_full = [], 0, 0, set(), 0
        for a, b, used in zip(la.tolist(), lb.tolist(), auto["band_used"].tolist()):
            w, k = w0, 0
            while worth(a, b, w) and (used == NO_BAND or w <= used):
                if len(rounds) <= k:
                    rounds.append(0)
                rounds[k] += 1
                filled += cells_filled(a, b, w)
                in_band += cells_in_band(a, b, w)
                variants.add(cols_of(a, b, w))
                w, k = 2 * w, k + 1
            if used == NO_BAND:
                to_full += 1
                filled += full_filled(a, b)
        print(json.dumps({"shape": name, "call": "msc_align_pairs_auto", "first_band": w0, "seconds": round(med["auto"], 6), "speedup": round(med["full"] / med["auto"], 3),
                          "cells_filled": filled, "cells_in_band": in_band, "cells_grid": grid, "cells_filled_per_s": round(filled / med["auto"]), "pairs_per_round": rounds,
                          "pairs_to_the_full_kernel": to_full, "columns_per_lane": sorted(variants), "kernel": ctx.last_kernel_info()[0]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
