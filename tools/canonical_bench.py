#!/usr/bin/env python3
"""msc_hist_canonical_batch next to msc_hist_revcomp_batch on the same slots -- run on the GPU box.
    python tools/canonical_bench.py [n_dense] [n_sparse] [reps] [--profile DIR]
The operator out of place and in place on n_dense (default 100 000) dense slots of k = 9 / uint32_t (1 MiB a slot) and on n_sparse (default
100 000) sparse slots of the same 1 kb family sequences, beside msc_hist_revcomp_batch of the same slots into the same destination: the kernel
the canonical one mirrors, and the yardstick for its byte rate. The calls alternate in one process; device-synchronised wall clock (every call
ends in a stream wait), one warm-up each, the median of `reps` (default 5). A sparse destination is cleared before every call, outside the clock;
the in-place form on a sparse set appends to the set it reads, so that set is rebuilt before every call, outside the clock too.
Bytes, dense: 2 x slot bytes per slot for both operators (the canonical kernel reads a tile once per tile written: it handles a tile and its
partner in one work item); the whole call also runs msc_launch_finalize, which reads every new slot once more -- `finalize_read_bytes`.
In place the dense operator is applied to its own result again on every repetition (the counts grow; the work does not change).
Last line: what --canonical adds to msc_cluster's build stage -- chunks of 8 192 sequences built (msc_hist_build_packed) and made canonical in
place, the two parts timed separately.
--profile DIR: afterwards the dense calls once more in a child process under `rocprofv3 --kernel-trace --stats` (a run of its own).
One JSON line per measurement. No ratio is a gate."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

argv = sys.argv[1:]
profile_dir = None
if "--profile" in argv:
    i = argv.index("--profile")
    profile_dir = argv[i + 1]
    del argv[i:i + 2]
n_dense = int(argv[0]) if len(argv) > 0 else 100000
n_sparse = int(argv[1]) if len(argv) > 1 else 100000
reps = int(argv[2]) if len(argv) > 2 else 5

import numpy as np
from meshclust2_amd import api, synth

ctx = api.Context(0)
K, BITS = 9, 32


def fill(hs, codes, first=0):
    for off in range(0, len(codes), 8192):
        part = codes[off:off + 8192]
        b = synth.pack_batch(part)
        hs.build_packed(first + off, len(part), b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"])


def timed(fn, before=None):
    if before:
        before()
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return time.perf_counter() - t0


def medians(calls, before=None):
    """the calls alternating: -> the median seconds of each"""
    for c in calls:
        timed(c, before)          # warm-up: code objects, scratch
    t = [[] for _ in calls]
    for _ in range(reps):
        for i, c in enumerate(calls):
            t[i].append(timed(c, before))
    return [float(np.median(x)) for x in t]


def dense():
    if n_dense == 0:
        return
    codes, _ = synth.family_codes(2026, n_dense, 1000, family=20)
    src = api.HistogramSet(ctx, K, BITS, n_dense)
    dst = api.HistogramSet(ctx, K, BITS, n_dense)
    fill(src, codes)
    ids = np.arange(n_dense, dtype=np.uint32)
    names = []
    def call(f):
        def run():
            f()
            names.append(ctx.last_kernel_info()[0])
        return run
    t_rc, t_out, t_in = medians([call(lambda: dst.revcomp_batch(ids, src, ids)), call(lambda: dst.canonical_batch(ids, src, ids)),
                                 call(lambda: src.canonical_batch(ids, src, ids))])
    slot = (4 ** K) * (BITS // 8)
    nbytes = 2 * n_dense * slot
    print(json.dumps(dict(what="operator", layout="dense", k=K, bits=BITS, slots=n_dense, bytes_moved=nbytes, finalize_read_bytes=n_dense * slot, revcomp_batch_s=t_rc,
                          canonical_out_of_place_s=t_out, canonical_in_place_s=t_in, revcomp_GBps=nbytes / t_rc / 1e9, canonical_out_of_place_GBps=nbytes / t_out / 1e9,
                          canonical_in_place_GBps=nbytes / t_in / 1e9, out_of_place_over_revcomp=t_out / t_rc, in_place_over_revcomp=t_in / t_rc,
                          kernels=sorted(set(names)))), flush=True)
    src.close(); dst.close()


def sparse():
    if n_sparse == 0:
        return
    codes, _ = synth.family_codes(2026, n_sparse, 1000, family=20)
    entries = sum(c.size for c in codes) + 1024
    src = api.HistogramSet(ctx, K, BITS, n_sparse, sparse_entries=entries)
    dst = api.HistogramSet(ctx, K, BITS, n_sparse, sparse_entries=2 * entries)
    own = api.HistogramSet(ctx, K, BITS, n_sparse, sparse_entries=3 * entries)
    fill(src, codes)
    ids = np.arange(n_sparse, dtype=np.uint32)
    t_rc, t_out = medians([lambda: dst.revcomp_batch(ids, src, ids), lambda: dst.canonical_batch(ids, src, ids)], before=dst.clear)
    kernel = ctx.last_kernel_info()[0]

    def refill():
        own.clear()
        own.copy_batch(ids, src, ids)
    t_in, = medians([lambda: own.canonical_batch(ids, own, ids)], before=refill)
    step = max(1, n_sparse // 1000)
    stored = sum(src.entries(i) for i in range(0, n_sparse, step)) * step          # (sampled)
    merged = sum(own.entries(i) for i in range(0, n_sparse, step)) * step
    print(json.dumps(dict(what="operator", layout="sparse", k=K, bits=BITS, slots=n_sparse, stored_bins_about=stored, merged_bins_about=merged,
                          revcomp_bytes_about=2 * 12 * stored, canonical_bytes_about=12 * (stored + merged), revcomp_batch_s=t_rc, canonical_out_of_place_s=t_out,
                          canonical_in_place_s=t_in, out_of_place_over_revcomp=t_out / t_rc, in_place_over_revcomp=t_in / t_rc, kernel=kernel)), flush=True)
    src.close(); dst.close(); own.close()


def build_stage():
    """what msc_cluster --canonical adds to the build stage: per chunk of 8 192 points, get_points and then the operator in place"""
    n = min(n_dense, 32768) or min(n_sparse, 32768)
    if n == 0:
        return
    codes, _ = synth.family_codes(2026, n, 1000, family=20)
    for layout in ("dense", "sparse"):
        hs = api.HistogramSet(ctx, K, BITS, n, sparse_entries=3 * sum(c.size for c in codes) + 1024 if layout == "sparse" else 0)
        t_build = t_canon = 0.0
        for rep in range(2):          # (the first pass warms up)
            if layout == "sparse":
                hs.clear()
            t_build = t_canon = 0.0
            for off in range(0, n, 8192):
                part = codes[off:off + 8192]
                b = synth.pack_batch(part)
                t_build += timed(lambda: hs.build_packed(off, len(part), b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"]))
                s = np.arange(off, off + len(part), dtype=np.uint32)
                t_canon += timed(lambda: hs.canonical_batch(s, hs, s))
        print(json.dumps(dict(what="build stage", layout=layout, k=K, bits=BITS, points=n, chunk=8192, build_s=t_build, canonical_s=t_canon, added=t_canon / t_build)), flush=True)
        hs.close()


dense()
sparse()
build_stage()
ctx.close()
if profile_dir:
    os.makedirs(profile_dir, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", profile_dir, "--", sys.executable, os.path.abspath(__file__), str(min(n_dense, 4096)), "20000", "2"],
                   check=False, timeout=600)
