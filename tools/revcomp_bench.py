#!/usr/bin/env python3
"""msc_hist_revcomp_batch and msc_search_pairs_strands next to their yardsticks -- run on the GPU box.
    python tools/revcomp_bench.py [op|search|all] [n_slots] [n_sparse] [n_q] [m] [reps] [--profile DIR]
op      the operator on n_slots (default 1 024) dense slots of k = 9 / uint32_t and of k = 10 / uint8_t (1 MiB a slot: n_slots MiB read and as
        many written) and on n_sparse (default 100 000) sparse slots of 1 kb sequences at k = 9 / uint32_t, against msc_hist_copy_batch of the
        same slots: unchanged code that moves the same bytes. The two calls alternate in one process; device-synchronised wall clock (both calls
        end in a stream wait), one warm-up each, the median of `reps` (default 9). A sparse destination is cleared before every call, outside the
        clock. Bytes: 2 x slot bytes per dense slot; 2 x 12 bytes per stored bin per sparse slot (entry + cum).
search  msc_search_pairs_strands on n_q (default 8 192) queries x m (default 100 000) candidates, k = 9 / uint32_t, 1 kb family sequences as
        bench.py makes them, tests/golden/weights_k9_u32_fc.txt, dense and sparse with msc_set_sparse_matrix_pass, next to msc_search_pairs on
        the same inputs (the yardstick is twice its time) and to msc_hist_revcomp_batch of the n_q queries alone. The merge is what is left:
        strands - 2 x plain - revcomp (derived, not timed on its own).
--profile DIR: afterwards the dense operator once more in a child process under `rocprofv3 --kernel-trace --stats` (a run of its own).
One JSON line per measurement. Targets, not gates: the operator within 2 x the copy, the search within 1.15 x twice the plain search."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

argv = sys.argv[1:]
profile_dir = None
if "--profile" in argv:
    i = argv.index("--profile")
    profile_dir = argv[i + 1]
    del argv[i:i + 2]
what = argv[0] if len(argv) > 0 else "all"
n_slots = int(argv[1]) if len(argv) > 1 else 1024
n_sparse = int(argv[2]) if len(argv) > 2 else 100000
n_q = int(argv[3]) if len(argv) > 3 else 8192
m = int(argv[4]) if len(argv) > 4 else 100000
reps = int(argv[5]) if len(argv) > 5 else 9

import numpy as np
from meshclust2_amd import api, synth
from golden_util import weights_text

ctx = api.Context(0)


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


def median_pair(a, b, before=None):
    """two calls alternating: -> (median seconds of a, of b)"""
    timed(a, before); timed(b, before)          # warm-up: code objects, scratch
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a, before))
        tb.append(timed(b, before))
    return float(np.median(ta)), float(np.median(tb))


def operator():
    for k, bits in ((9, 32), (10, 8)):
        codes, _ = synth.family_codes(2026, n_slots, 1000, family=20)
        src = api.HistogramSet(ctx, k, bits, n_slots)
        dst = api.HistogramSet(ctx, k, bits, n_slots)
        fill(src, codes)
        ids = np.arange(n_slots, dtype=np.uint32)
        t_copy, t_rc = median_pair(lambda: dst.copy_batch(ids, src, ids), lambda: dst.revcomp_batch(ids, src, ids))
        nbytes = 2 * n_slots * (4 ** k) * (bits // 8)
        print(json.dumps(dict(what="operator", layout="dense", k=k, bits=bits, slots=n_slots, bytes_moved=nbytes, copy_batch_s=t_copy, revcomp_batch_s=t_rc,
                              ratio=t_rc / t_copy, copy_GBps=nbytes / t_copy / 1e9, revcomp_GBps=nbytes / t_rc / 1e9, kernel=ctx.last_kernel_info()[0])), flush=True)
        src.close(); dst.close()
    k, bits = 9, 32
    codes, _ = synth.family_codes(2026, n_sparse, 1000, family=20)
    entries = sum(c.size for c in codes) + 1024
    src = api.HistogramSet(ctx, k, bits, n_sparse, sparse_entries=entries)
    dst = api.HistogramSet(ctx, k, bits, n_sparse, sparse_entries=entries)
    fill(src, codes)
    ids = np.arange(n_sparse, dtype=np.uint32)
    t_copy, t_rc = median_pair(lambda: dst.copy_batch(ids, src, ids), lambda: dst.revcomp_batch(ids, src, ids), before=dst.clear)
    stored = sum(src.entries(i) for i in range(0, n_sparse, max(1, n_sparse // 1000))) * max(1, n_sparse // 1000)          # (sampled)
    nbytes = 2 * 12 * stored
    print(json.dumps(dict(what="operator", layout="sparse", k=k, bits=bits, slots=n_sparse, stored_bins_about=stored, bytes_moved_about=nbytes, copy_batch_s=t_copy,
                          revcomp_batch_s=t_rc, ratio=t_rc / t_copy, kernel=ctx.last_kernel_info()[0])), flush=True)
    src.close(); dst.close()


def search():
    pred = api.Predictor.from_text(ctx, weights_text("weights_k9_u32_fc.txt"))
    codes, _ = synth.family_codes(2026, m, 1000, family=20)
    q = np.linspace(0, m - 1, n_q).astype(np.uint32)
    qids = np.arange(n_q, dtype=np.uint32)
    for layout in ("dense", "sparse-matrix"):
        sparse = layout != "dense"
        entries = sum(c.size for c in codes) + 1024 if sparse else 0
        hs = api.HistogramSet(ctx, 9, 32, m, sparse_entries=entries)
        fill(hs, codes)
        turned = api.HistogramSet(ctx, 9, 32, n_q, sparse_entries=n_q * 1100 if sparse else 0)
        ctx.set_sparse_matrix_pass(sparse)
        got = {}
        t_plain, t_strands = median_pair(lambda: got.__setitem__("plain", pred.search_pairs(hs, None, hs, q, m=m)),
                                         lambda: got.__setitem__("strands", pred.search_pairs_strands(hs, None, hs, q, m=m)))
        t_rc = float(np.median([timed(lambda: turned.revcomp_batch(qids, hs, q), before=turned.clear if sparse else None) for _ in range(reps)]))
        ctx.set_sparse_matrix_pass(False)
        print(json.dumps(dict(what="search", layout=layout, n_q=n_q, m=m, plain_s=t_plain, strands_s=t_strands, revcomp_queries_s=t_rc,
                              merge_and_rest_s=t_strands - 2 * t_plain - t_rc, ratio_to_twice_plain=t_strands / (2 * t_plain),
                              pairs_plain=got["plain"][3]["n_pairs"], pairs_strands=got["strands"][4]["n_pairs"], route=got["strands"][4]["route"],
                              reverse_strand_pairs=int(got["strands"][3].sum()))), flush=True)
        hs.close(); turned.close()


if what in ("op", "all"):
    operator()
if what in ("search", "all"):
    search()
ctx.close()
if profile_dir:
    os.makedirs(profile_dir, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", profile_dir, "--", sys.executable, os.path.abspath(__file__), "op", str(n_slots), "1000", "0", "0", "2"],
                   check=False, timeout=600)
