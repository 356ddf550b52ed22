#!/usr/bin/env python3
"""msc_align_pairs_long / _long_auto on synthetic pairs -- run on the GPU box.

    python tools/align_long_bench.py [--reps 5] [--rows 256,512,1024,2048] [--skip-large]

One JSON line per measurement: the median wall time of `reps` calls after a warm-up call (a call uploads the sequences, runs the kernels and
brings the integers back), the fastest and the slowest call (the run-to-run spread), cells per second at the median, and the kernel
msc_last_kernel_info named. Pairs are a template and a mutated copy of it (meshclust2_amd/synth.py). What it measures (profiles/align_long.md
keeps what it printed):

  yardstick   msc_align_pairs on 200 pairs of 20 kb: one wave a pair, packed states, no borders
  full grid   msc_align_pairs_long on 1, 16 and 200 pairs of 50 kb, per tile height
  one pair    a single 32 767 x 32 767 pair through msc_align_pairs (one wave) and through msc_align_pairs_long under MSC_ALIGN_LONG_ALL=1
              (the tiles), per tile height: the new route must be faster by more than the spread of the old one
  auto        200 pairs of 50 kb at 95 % and at 99 % through msc_align_pairs_long_auto, per tile height: time and the distribution of band_used
              (the full grid of the same cells: the 200-pair line above)
  short       20 000 pairs of 1 kb through msc_align_pairs and through msc_align_pairs_long, which routes them to the same kernels"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshclust2_amd import api, synth          # noqa: E402


def similar_pairs(n_pairs, length, seed, sub_rate, indel_rate):
    seqs = []
    for p in range(n_pairs):
        t = synth.template(seed, p, length)
        seqs += [synth.to_ascii(t), synth.to_ascii(synth.member(seed, p, 0, t, sub_rate=sub_rate, indel_rate=indel_rate))]
    return seqs, np.arange(0, 2 * n_pairs, 2, dtype=np.uint32), np.arange(1, 2 * n_pairs, 2, dtype=np.uint32)


def timed(ctx, what, call, cells, reps, **more):
    call()          # warm-up: scratch buffers, code object
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        r = call()
        times.append(time.perf_counter() - t)
    med = float(np.median(times))
    line = dict(what=what, cells=cells, reps=reps, median_s=round(med, 6), min_s=round(min(times), 6), max_s=round(max(times), 6), cells_per_s=round(cells / med),
                kernel=ctx.last_kernel_info()[0], **more)
    print(json.dumps(line), flush=True)
    return r, times


def cells_of(seqs, first, second):
    ln = np.array([len(s) for s in seqs], dtype=np.int64)
    return int((ln[first] * ln[second]).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="256,512,1024,2048")
    ap.add_argument("--skip-large", action="store_true", help="leave out the 200-pair lists of 50 kb")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    heights = [int(v) for v in args.rows.split(",")]
    for k in ("MSC_ALIGN_LONG_ALL", "MSC_ALIGN_TILE_ROWS"):
        os.environ.pop(k, None)
    ctx = api.Context(args.device)

    seqs, first, second = similar_pairs(200, 20000, 301, 0.03, 0.005)
    timed(ctx, "yardstick: msc_align_pairs, 200 x 20 kb", lambda: api.align_pairs(ctx, seqs, first, second), cells_of(seqs, first, second), args.reps)

    seqs, first, second = similar_pairs(1, 32767, 303, 0.03, 0.005)
    seqs = [s[:32767].ljust(32767, b"A") for s in seqs]
    cells = cells_of(seqs, first, second)
    old, old_times = timed(ctx, "one pair 32767 x 32767: msc_align_pairs (one wave)", lambda: api.align_pairs(ctx, seqs, first, second), cells, args.reps)
    os.environ["MSC_ALIGN_LONG_ALL"] = "1"
    for h in heights:
        os.environ["MSC_ALIGN_TILE_ROWS"] = str(h)
        new, new_times = timed(ctx, "one pair 32767 x 32767: msc_align_pairs_long, tiles", lambda: api.align_pairs_long(ctx, seqs, first, second), cells, args.reps, tile_rows=h)
        assert all((new[k] == old[k]).all() for k in ("score", "length", "matches"))
        print(json.dumps(dict(what="one pair: old / new", tile_rows=h, ratio_of_medians=round(float(np.median(old_times) / np.median(new_times)), 2),
                              old_spread_s=round(max(old_times) - min(old_times), 6), gain_s=round(float(np.median(old_times) - np.median(new_times)), 6),
                              faster_by_more_than_the_old_spread=bool(np.median(old_times) - max(new_times) > max(old_times) - min(old_times)))), flush=True)
    del os.environ["MSC_ALIGN_LONG_ALL"]

    for n_pairs in (1, 16) + (() if args.skip_large else (200,)):
        seqs, first, second = similar_pairs(n_pairs, 50000, 305, 0.03, 0.005)
        for h in heights:
            os.environ["MSC_ALIGN_TILE_ROWS"] = str(h)
            timed(ctx, "full grid: msc_align_pairs_long, %d x 50 kb" % n_pairs, lambda: api.align_pairs_long(ctx, seqs, first, second), cells_of(seqs, first, second), args.reps,
                  tile_rows=h)

    for name, sub_rate, indel_rate in (("95 %", 0.04, 0.01), ("99 %", 0.008, 0.002)):
        seqs, first, second = similar_pairs(16 if args.skip_large else 200, 50000, 307, sub_rate, indel_rate)
        for h in heights:
            os.environ["MSC_ALIGN_TILE_ROWS"] = str(h)
            r, _ = timed(ctx, "auto: msc_align_pairs_long_auto, %d x 50 kb at %s" % (first.size, name), lambda: api.align_pairs_long_auto(ctx, seqs, first, second),
                         cells_of(seqs, first, second), args.reps, tile_rows=h)
        bands, counts = np.unique(r["band_used"], return_counts=True)
        print(json.dumps(dict(what="auto: band_used at %s" % name, bands={str(int(b)): int(c) for b, c in zip(bands, counts)}, mean_identity=round(float(r["identity"].mean()), 4))), flush=True)
    del os.environ["MSC_ALIGN_TILE_ROWS"]

    seqs, _ = synth.families(309, 2000, 1000, family=20)
    first = np.arange(20000, dtype=np.uint32) % 2000
    second = ((first // 20) * 20 + (first % 20 + 1 + (np.arange(20000) // 2000) % 18) % 20).astype(np.uint32)
    cells = cells_of(seqs, first, second)
    for rep in range(2):          # the two calls take turns, so that a drift of the box shows in both
        timed(ctx, "short: msc_align_pairs, 20000 x 1 kb (turn %d)" % rep, lambda: api.align_pairs(ctx, seqs, first, second), cells, args.reps)
        timed(ctx, "short: msc_align_pairs_long, 20000 x 1 kb (turn %d)" % rep, lambda: api.align_pairs_long(ctx, seqs, first, second), cells, args.reps)
    ctx.close()


if __name__ == "__main__":
    main()
