#!/usr/bin/env python3
"""msc_align_pairs_trace beside msc_align_pairs on synthetic pairs -- run on the GPU box.

    python tools/align_trace_bench.py [--reps 3] [--trace-bytes N]

Two shapes of tools/align_bench.py, built the same way (members of one family against each other: 3 % substitutions, 0.5 % indels): 20 000 pairs
of 1 kb and 200 pairs of 20 kb. Per shape, in one process and on one context, after a warm-up call of each: `reps` rounds that time
api.align_pairs (the yardstick, unchanged) and api.align_pairs_trace (the call and the fetch of the whole op list) one after the other, host
clock around calls that end in a device synchronise. One JSON line per shape: the best wall time of each, their ratio, and of the best trace
call the split msc_last_kernel_ms gives -- forward_ms (the k_align_pairs_dirs launches, HIP events around each group's), device_ms (first
launch to last walk) and walk_and_gaps_ms = device_ms - forward_ms (both walks, the scan's round trip per group and whatever the list's growth
cost) -- with the groups the call was dealt into, the bytes of back pointers and the runs returned. The triples of the two calls are compared.
--trace-bytes sets MSC_ALIGN_TRACE_BYTES for the trace calls (0: the library's 2 GiB)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshclust2_amd import api          # noqa: E402
from align_bench import pairs_of        # noqa: E402

SHAPES = [("20000 x 1 kb", 20000, 1000), ("200 x 20 kb", 200, 20000)]
DEFAULT_CAP = 2 << 30


def groups_of(la, lb, cap):
    """the groups msc_align_pairs_trace deals a list into -> (groups, bytes of back pointers)"""
    need = ((la + 255) // 256) * (lb + 63) * 128
    groups, held = 1, 0
    for b in need.tolist():
        if held and held + b > cap:
            groups, held = groups + 1, 0
        held += b
    return groups, int(need.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace-bytes", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.trace_bytes:
        os.environ["MSC_ALIGN_TRACE_BYTES"] = str(args.trace_bytes)
    ctx = api.Context(args.device)
    for name, n_pairs, length in SHAPES:
        seqs, first, second = pairs_of(n_pairs, length, 77 + length)
        ln = np.array([len(s) for s in seqs], dtype=np.int64)
        cells = int((ln[first] * ln[second]).sum())
        groups, dir_bytes = groups_of(ln[first], ln[second], args.trace_bytes or DEFAULT_CAP)
        plain = api.align_pairs(ctx, seqs, first, second)          # warm-up: scratch buffers, code objects
        traced = api.align_pairs_trace(ctx, seqs, first, second)
        same = all(np.array_equal(plain[k], traced[k]) for k in ("score", "length", "matches"))
        best_plain = best_trace = None
        split = (0.0, 0.0)
        for _ in range(args.reps):
            t = time.perf_counter()
            api.align_pairs(ctx, seqs, first, second)
            dt = time.perf_counter() - t
            best_plain = dt if best_plain is None else min(best_plain, dt)
            t = time.perf_counter()
            traced = api.align_pairs_trace(ctx, seqs, first, second)
            dt = time.perf_counter() - t
            if best_trace is None or dt < best_trace:
                best_trace, split = dt, ctx.last_kernel_ms()
        forward_ms, device_ms = split
        print(json.dumps({"shape": name, "pairs": n_pairs, "cells": cells, "align_pairs_s": round(best_plain, 6), "align_pairs_trace_s": round(best_trace, 6),
                          "trace_over_plain": round(best_trace / best_plain, 3), "forward_ms": round(forward_ms, 3), "device_ms": round(device_ms, 3),
                          "walk_and_gaps_ms": round(device_ms - forward_ms, 3), "walk_share_of_device": round((device_ms - forward_ms) / device_ms, 4),
                          "plain_cells_per_s": round(cells / best_plain), "forward_cells_per_s": round(cells / (forward_ms * 1e-3)), "groups": groups,
                          "direction_bytes": dir_bytes, "runs": int(traced["op_offsets"][-1]), "triples_equal": bool(same), "kernel": ctx.last_kernel_info()[0]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
