"""A fixed table of small msc_score_multi calls, one JSON line per call: the kernel the call named (msc_last_kernel_info), its launches,
whether msc_last_close_counts kept the call's counts, and a SHA-256 of every output array. Two builds of the library that take the same
routes and compute the same values print the same lines; tests/golden/qxm_routes.json holds the lines of the build before msc_score_multi
became a block plan with one function per route, and tests/test_gpu_qxm_routes.py compares a fresh run with them.

    python tools/qxm_routes.py [--lib PATH/libmeshclust2_hip.so] [--dump DIR]

The table: the shapes of tests/ring_variant_check.py (32-bit k = 9, 64-bit k = 6; digest, ring, raw tiles, matrix cores), three dense k = 7
sets and two sparse sets (with and without msc_set_sparse_matrix_pass) at n_q = 2, 64, 65, 129, 130, 257 over a slot list and over a range,
and a `--feat slow` model (jensen_shannon: the divergence sums ride behind the streaming kernel). The slow model's weighted sums hold FP64
divergence sums and are not hashed: --dump DIR writes them as .npy files to be compared with a tolerance.

    python tools/qxm_routes.py --flags [--lib PATH/libmeshclust2_hip.so]

A second table, of calls that ask for the close flags alone (want = close, counts) with an earth_movers_distance model: the tails of a
matrix-core block that the first table never reaches -- the bound screen of the distance, the folded product, the second run of a block
whose folded list overflowed. A line holds the kernel, the launches, a SHA-256 of the flags and of the counts, msc_last_emd_walk and
msc_last_fold_screen. tests/golden/qxm_flag_routes.json holds the lines of the build before run_matrix became a driver over stage
functions."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
NQS = (2, 64, 65, 129, 130, 257)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def flag_table(ctx, api, synth):
    """the flags-only calls: one JSON line each. A fresh Feature per case (a model remembers that its lists overflowed) unless the case is
    about that memory."""
    text = open(os.path.join(GOLDEN, "weights_k9_u32.txt")).read()
    lines = []

    def call(case, feat, cands, slots, qset, qs, m=None):
        got = api.score_multi(ctx, feat, cands, slots, qset, qs, m=m, want=("close", "counts"))
        lines.append(json.dumps(dict(case=case, kernel=ctx.last_kernel_info()[0], launches=ctx.last_kernel_launches(), emd_walk=ctx.last_emd_walk(),
                                     fold_screen=ctx.last_fold_screen(), sha=dict(close=sha(got["close"]), counts=sha(got["counts"]))), sort_keys=True))
        return got

    def fresh():
        return api.Feature.from_text(ctx, text, 0)

    def shifted(by):          # the model with its intercept (the line after the first `n_combos:`) lowered by `by`
        ls = text.splitlines()
        at = next(i for i, ln in enumerate(ls) if ln.startswith("n_combos:")) + 1
        ls[at] = repr(float(ls[at]) - float(by))
        return api.Feature.from_text(ctx, "\n".join(ls) + "\n", 0)

    # the set of tests/test_gpu_fold_screen.py: 640 sequences of 1 000 bases in families of four, k = 9, 32-bit
    seqs = synth.families(20260002, 640, 1000, family=4)[0]
    n = len(seqs)
    hs = api.HistogramSet(ctx, 9, 32, n)
    hs.build(seqs)
    qs = np.arange(200, dtype=np.uint32)
    call("200 x 640 range: two queued blocks, piped, folded", fresh(), hs, None, hs, qs, m=n)
    call("200 x 640 shuffled slot list", fresh(), hs, np.random.default_rng(7).permutation(n).astype(np.uint32), hs, qs)
    ctx.set_fold_screen(0)
    call("fold screen off: the unfolded bound tail", fresh(), hs, None, hs, qs, m=n)
    ctx.set_fold_screen(16)
    ctx.set_emd_bounds(False)
    call("emd bounds off: the scored tail, dense walk", fresh(), hs, None, hs, qs, m=n)
    ctx.set_emd_bounds(True)
    ctx.set_block_pipe(False)
    call("block pipe off: queued on one stream", fresh(), hs, None, hs, qs, m=n)
    ctx.set_block_pipe(True)
    ctx.set_kernel_timing(False)
    call("kernel timing off: queued without timing events", fresh(), hs, None, hs, qs, m=n)
    ctx.set_kernel_timing(True)
    call("3 x 200: one block, not queued", fresh(), hs, None, hs, np.array([3, 129, 130], dtype=np.uint32), m=200)
    call("3 x 20: under 64 pairs, no list", fresh(), hs, None, hs, np.array([3, 129, 130], dtype=np.uint32), m=20)
    hs.close()
    # the set of tests/test_gpu_emd_bounds.py (families of 20): every folded list overflows and the blocks run again, unfolded; the model
    # is remembered for it. Then with the intercept moved by the median sum of all pairs: the unfolded lists overflow too (the dense walk)
    seqs = synth.families(20260002, 800, 1000)[0]
    n = len(seqs)
    hs = api.HistogramSet(ctx, 9, 32, n)
    hs.build(seqs)
    qs = np.arange(130, dtype=np.uint32)
    feat = fresh()
    call("families of 20, 130 x 800, first call", feat, hs, None, hs, qs, m=n)
    call("families of 20, 130 x 800, second call: model remembered", feat, hs, None, hs, qs, m=n)
    sums = api.score_multi(ctx, feat, hs, None, hs, qs, m=n, want=("sum",))["sum"]
    feat = shifted(np.median(sums))
    call("families of 20, intercept at the median, first call", feat, hs, None, hs, qs, m=n)
    call("families of 20, intercept at the median, second call: model remembered", feat, hs, None, hs, qs, m=n)
    hs.close()
    # two sparse sets, mirrors from the lists
    seqs = synth.families(20260002, 640, 1000, family=4)[0]
    sp = api.HistogramSet(ctx, 9, 32, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 1024)
    sp.build(seqs)
    sq = api.HistogramSet(ctx, 9, 32, 130, sparse_entries=sum(len(s) for s in seqs[:130]) + 1024)
    sq.build(seqs[:130])
    ctx.set_sparse_matrix_pass(True)
    call("two sparse sets, 130 x 640", fresh(), sp, None, sq, np.arange(130, dtype=np.uint32), m=len(seqs))
    ctx.set_sparse_matrix_pass(False)
    sq.close()
    sp.close()
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flags", action="store_true", help="the second table: flags-only calls (the bound and folded tails of a matrix-core block)")
    ap.add_argument("--lib", help="run against this build of the library instead of the tree's")
    ap.add_argument("--dump", help="directory for the arrays that are not hashed")
    args = ap.parse_args()
    from meshclust2_amd import _capi
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    from meshclust2_amd import api, synth
    ctx = api.Context(0)
    if args.flags:
        flag_table(ctx, api, synth)
        ctx.close()
        return
    lines = []

    def call(case, feat, hs, cands, qs, m=None, feat_mask=api.FEAT_FAST, hashed=("sum", "csum", "close", "raw"), dumped=()):
        got = api.score_multi(ctx, feat, hs, cands, hs, qs, m=m, feat_mask=feat_mask, want=("sum", "csum", "close"))
        kernel, tile = ctx.last_kernel_info()
        launches = ctx.last_kernel_launches()
        counts = np.zeros(len(qs), dtype=np.uint64)
        kept = ctx.lib.msc_last_close_counts(ctx.h, counts.ctypes.data_as(_capi.C.c_void_p), len(qs)) == 0
        rec = dict(case=case, kernel=kernel, query_tile=tile, launches=launches, counts_kept=kept, sha={k: sha(got[k]) for k in hashed if got[k] is not None})
        if kept:
            rec["sha"]["counts"] = sha(counts)
        for k in dumped:
            if args.dump:
                os.makedirs(args.dump, exist_ok=True)
                np.save(os.path.join(args.dump, "%03d_%s.npy" % (len(lines), k)), got[k])
        lines.append(json.dumps(rec, sort_keys=True))

    text = open(os.path.join(GOLDEN, "weights_k9_u32.txt")).read()
    feat = api.Feature.from_text(ctx, text, 0)
    # the shapes of tests/ring_variant_check.py
    for dtype, k, n, length in ((32, 9, 330, 1000), (64, 6, 700, 300)):
        seqs, _ = synth.families(900 + k, n, length, family=10)
        hs = api.HistogramSet(ctx, k, dtype, len(seqs))
        hs.build(seqs)
        for nq, cands in ((4, np.arange(n)), (9, np.arange(5, n)), (16, np.arange(n - 1, -1, -1)), (8, np.array([7])), (5, np.array([3, 9, 4])),
                          (40, np.arange(n)), (64, np.arange(3, n)), (33, np.arange(n - 1, 100, -1))):
            call("ring u%d k%d nq%d m%d" % (dtype, k, nq, cands.size), feat, hs, cands.astype(np.uint32), (np.arange(nq, dtype=np.uint32) * 3) % n)
        for nq in (129, 257):          # short hot lists: the 32-bit set's blocks of 128 stay on the matrix cores, queued ahead of the trailing single query
            call("ring u%d k%d nq%d range" % (dtype, k, nq), feat, hs, None, (np.arange(nq, dtype=np.uint32) * 3) % n, m=n - 7)
        hs.close()
    # dense k = 7 sets: counts of 3 .. 8 in most tiles; every block count of the plan, a slot list and a range
    seqs, _ = synth.families(913, 150, 3000, family=10)
    n = len(seqs)
    for dtype in (16, 8, 32):
        hs = api.HistogramSet(ctx, 7, dtype, n)
        hs.build(seqs)
        for nq in NQS:
            qs = (np.arange(nq, dtype=np.uint32) * 7) % n
            call("dense u%d k7 nq%d list" % (dtype, nq), feat, hs, np.arange(n - 1, 2, -1, dtype=np.uint32), qs)
            call("dense u%d k7 nq%d range" % (dtype, nq), feat, hs, None, qs, m=n - 10)
        hs.close()
    # two sparse sets, with and without the matrix-core pass; the second one's tandem repeats make long hot lists: blocks decline
    rng = np.random.default_rng(57)
    plain, _ = synth.families(5307, 140, 600, family=5, length_jitter=40)
    reps = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=150)) * 4 for _ in range(100)]
    mixed = [bytes(s) for s in plain] + reps
    seqs9, _ = synth.families(5301, 150, 1000, family=6, length_jitter=100)
    for name, k, sq in (("plain k9", 9, [bytes(s) for s in seqs9]), ("repeats k7", 7, mixed)):
        f = api.Feature.from_text(ctx, text.replace("k: 9", "k: %d" % k), 0)
        sp = api.HistogramSet(ctx, k, 32, len(sq), sparse_entries=sum(len(s) for s in sq) + 1024)
        sp.build(sq)
        for on in (False, True):
            ctx.set_sparse_matrix_pass(on)
            for nq in NQS:
                # (repeats k7: 128 plain queries, then tandem-repeat ones, then plain ones again)
                qs = np.concatenate([np.arange(128), 140 + np.arange(100), np.arange(100, 140)])[:nq].astype(np.uint32) if k == 7 else (np.arange(nq, dtype=np.uint32) * 7) % len(sq)
                call("sparse %s %s nq%d list" % (name, "on" if on else "off", nq), f, sp, np.arange(len(sq) - 1, -1, -1, dtype=np.uint32), qs)
                call("sparse %s %s nq%d range" % (name, "on" if on else "off", nq), f, sp, None, qs, m=len(sq) - 3)
        ctx.set_sparse_matrix_pass(False)
        sp.close()
    # a `--feat slow` model: the flags are hashed, the sums (they hold the two FP64 divergence sums) are dumped
    slow = api.Feature.from_text(ctx, open(os.path.join(GOLDEN, "weights_cfg5_k9.txt")).read(), 0)
    seqs, _ = synth.families(5308, 140, 1000, family=5, length_jitter=100)
    hs = api.HistogramSet(ctx, 9, 8, len(seqs))
    hs.build(seqs)
    for nq in (2, 65, 130):
        call("slow u8 k9 nq%d" % nq, slow, hs, None, (np.arange(nq, dtype=np.uint32) * 3) % len(seqs), m=len(seqs), feat_mask=0, hashed=("close",), dumped=("sum", "csum"))
    hs.close()
    ctx.close()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
