"""A fixed table of small 1 x M calls, one JSON line per call: the kernel the call named (msc_last_kernel_info), its launches, the call's
status and a SHA-256 of every output array. Two builds of the library that take the same routes and compute the same values print the same
lines; tests/golden/score_routes.json holds the lines of the build before run_score became a route chosen in one place and one function
per stage, and tests/test_gpu_score_routes.py compares a fresh run with them.

    python tools/score_routes.py [--lib PATH/libmeshclust2_hip.so] [--dump DIR]

The table, in one fixed order (the rank lists of a set are built at the third pass that asks for them, so the order is part of a case):
dense sets without a list form (32-bit k = 6, 8-bit k = 3), the 64-bit range (k_pair_tiles_wide), a dense set with a sparse mirror (32-bit
k = 9: merge kernels, then the rank kernels, the streaming kernel behind msc_set_mirror_pass(0)), a sparse set (16-bit k = 9: whole-list
kernel, merge-path parts, rank kernels, the window call), the generic merge kernel (a count >= 2^16; 64-bit k = 13), a slot list one
entry longer than a chunk of the partial records, and the window call over a small dense set, fused and unfused. Outputs that hold the two FP64 divergence sums are not hashed: --dump DIR writes them
as .npy files to be compared bit for bit between two builds."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
# a chunk of a pass without a reduction: 256 MiB of partial records, 16 tiles (32-bit k = 7) of 24 bytes per candidate (run_score)
CHUNK_K7_U32 = (256 << 20) // (16 * 24)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class env:
    """a switch set for the calls inside the block only (the library reads these on every call)"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        os.environ[self.name] = "1"

    def __exit__(self, *exc):
        del os.environ[self.name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="run against this build of the library instead of the tree's")
    ap.add_argument("--dump", help="directory for the arrays that are not hashed")
    args = ap.parse_args()
    from meshclust2_amd import _capi
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    from meshclust2_amd import api, synth
    ctx = api.Context(0)
    lines = []

    def call(case, fn, div=False):
        """fn() -> dict of output arrays / numbers; div: the float outputs hold the two FP64 divergence sums (dumped, not hashed)"""
        status, got = 0, {}
        try:
            got = fn()
        except api.MscError as e:
            status = e.code
        kernel, tile = ctx.last_kernel_info()
        rec = dict(case=case, kernel=kernel, query_tile=tile, launches=ctx.last_kernel_launches(), status=status, sha={})
        for k, v in sorted(got.items()):
            a = np.asarray(v)
            if div and a.dtype == np.float64:
                if args.dump:
                    os.makedirs(args.dump, exist_ok=True)
                    np.save(os.path.join(args.dump, "%03d_%s.npy" % (len(lines), k)), a)
            else:
                rec["sha"][k] = sha(a)
        lines.append(json.dumps(rec, sort_keys=True))

    def raw(hs, slots, q, mask=api.FEAT_FAST, m=None):
        return lambda: dict(raw=api.pair_features_raw(ctx, hs, slots, hs, q, mask, m=m))

    def compute(feat, hs, slots, q, m=None):
        return lambda: feat.compute(hs, slots, hs, q, m=m)

    def get_close(trn, hs, slots, q, m=None):
        def fn():
            flags, bp, bs, im = trn.get_close(hs, slots, hs, q, m=m)
            return dict(flags=flags, best_pos=np.int64(bp), best_sim=np.float64(bs), any_close=np.int32(not im), n_close=np.uint64(flags.sum()))
        return fn

    def window(win, trn, first, end, hs, q):
        def fn():
            close, bp, bs, im = win.get_close(trn, first, end, hs, q)
            return dict(close_pos=np.sort(close), best_pos=np.int64(bp), best_sim=np.float64(bs), any_close=np.int32(not im), n_close=np.uint64(close.size))
        return fn

    fast9 = open(os.path.join(GOLDEN, "weights_k9_u32.txt")).read()
    slow9 = open(os.path.join(GOLDEN, "weights_cfg5_k9.txt")).read()
    models = []

    def model(text, k):
        models.append(api.Feature.from_text(ctx, text.replace("k: 9", "k: %d" % k), 0))
        return models[-1]

    groups = api.FEAT["sim_mm"] | api.FEAT["rre_k_r"]
    rep = np.array([5, 5, 0, 39, 7, 7, 7, 12, 0, 39, 1], dtype=np.uint32)          # a slot list with repeats

    # ---- dense, no list form: 32-bit k = 6 (16 KiB a histogram)
    seqs6, _ = synth.families(6101, 40, 300, family=5, length_jitter=20)
    hs = api.HistogramSet(ctx, 6, 32, len(seqs6) + 1)
    hs.build(seqs6)
    fast, slow = model(fast9, 6), model(slow9, 6)
    trn = api.Trainer(ctx, fast, 0.9)
    call("dense k6 raw range", raw(hs, None, 3, m=37))
    call("dense k6 raw list", raw(hs, rep, 2))
    call("dense k6 compute", compute(fast, hs, None, 1, m=40))
    call("dense k6 get_close", get_close(trn, hs, None, 0, m=40))
    with env("MSC_NO_FUSED_REDUCE"):
        call("dense k6 get_close unfused", get_close(trn, hs, None, 0, m=40))
    call("dense k6 get_close list", get_close(trn, hs, rep, 5))
    call("dense k6 filter", lambda: dict(keep=trn.filter(hs, 4, hs, rep)))
    call("dense k6 merge", lambda: dict(best=np.int64(trn.merge(hs, None, 10, 11, 30, n=40))))
    pred = api.Predictor.from_text(ctx, fast9.replace("k: 9", "k: 6"))
    call("dense k6 search", lambda: dict(zip(("close", "sim"), pred.search(hs, None, hs, 6, m=40))))
    call("dense k6 mean_nearest", lambda: dict(zip(("pos", "dist"), api.mean_nearest(ctx, hs, rep)[:2])))
    call("dense k6 slow compute", compute(slow, hs, None, 2, m=40), div=True)
    call("dense k6 slow get_close", get_close(api.Trainer(ctx, slow, 0.6), hs, rep, 5), div=True)
    call("dense k6 raw div", raw(hs, rep, 2, mask=api.FEAT_SLOW), div=True)
    call("dense k6 groups", raw(hs, rep, 2, mask=api.FEAT_FAST | groups))
    call("dense k6 m0 raw", raw(hs, None, 0, m=0))
    call("dense k6 m0 get_close", get_close(trn, hs, None, 0, m=0))
    # ---- wide: one count above 8 191
    hs.build([seqs6[0][:100] + b"A" * 9000 + seqs6[0][100:]], first_slot=40)
    wide_slots = np.array([40, 3, 40, 17, 0], dtype=np.uint32)
    call("wide k6 raw", raw(hs, wide_slots, 40))
    call("wide k6 get_close", get_close(api.Trainer(ctx, fast, 0.5), hs, None, 40, m=41))
    call("wide k6 compute", compute(fast, hs, None, 7, m=41))
    call("wide k6 slow compute", compute(slow, hs, wide_slots, 40), div=True)
    call("wide k6 mean_nearest", lambda: dict(zip(("pos", "dist"), api.mean_nearest(ctx, hs, wide_slots)[:2])))
    hs.close()
    # ---- 8-bit k = 3: padded histograms
    hs = api.HistogramSet(ctx, 3, 8, 40)
    hs.build(seqs6)
    f3 = model(fast9, 3)
    call("dense u8 k3 raw", raw(hs, rep, 2))
    call("dense u8 k3 compute", compute(f3, hs, None, 1, m=40))
    call("dense u8 k3 get_close", get_close(api.Trainer(ctx, f3, 0.9), hs, None, 0, m=40))
    call("dense u8 k3 slow compute", compute(model(slow9, 3), hs, None, 1, m=40), div=True)
    hs.close()

    # ---- dense with a mirror: 32-bit k = 9, and a 12 000-base sequence in slot 60
    seqs9, _ = synth.families(6102, 60, 1000, family=6, length_jitter=100)
    long9, _ = synth.families(6103, 24, 12000, family=4, length_jitter=500)
    fast, slow = model(fast9, 9), model(slow9, 9)
    trn, trn_slow = api.Trainer(ctx, fast, 0.9), api.Trainer(ctx, slow, 0.6)
    hs = api.HistogramSet(ctx, 9, 32, 62)
    hs.build(list(seqs9) + long9[:2])
    for i in range(4):          # the mirror's rank lists are built at the third pass that asks for them
        call("mirror k9 get_close %d" % (i + 1), get_close(trn, hs, None, i, m=60))
    with env("MSC_NO_RANKS_1XM"):
        call("mirror k9 get_close no ranks", get_close(trn, hs, None, 7, m=60))
    call("mirror k9 get_close list", get_close(trn, hs, rep, 8))
    call("mirror k9 raw", raw(hs, rep, 9))
    call("mirror k9 compute", compute(fast, hs, None, 10, m=62))
    call("mirror k9 slow compute", compute(slow, hs, None, 11, m=60), div=True)
    call("mirror k9 slow get_close", get_close(trn_slow, hs, rep, 12), div=True)
    with env("MSC_RANKS_DIV"):
        call("mirror k9 slow compute ranks div", compute(slow, hs, None, 11, m=60), div=True)
    call("mirror k9 groups", raw(hs, rep, 13, mask=api.FEAT_FAST | groups))
    call("mirror k9 long query raw", raw(hs, None, 60, m=62))
    call("mirror k9 long query get_close", get_close(api.Trainer(ctx, fast, 0.05), hs, None, 60, m=62))
    with env("MSC_NO_RANKS_ITEMS"):
        call("mirror k9 long query no items", raw(hs, None, 60, m=62))
    call("mirror k9 filter", lambda: dict(keep=trn.filter(hs, 4, hs, rep)))
    call("mirror k9 merge", lambda: dict(best=np.int64(trn.merge(hs, None, 10, 11, 30, n=60))))
    call("mirror k9 mean_nearest", lambda: dict(zip(("pos", "dist"), api.mean_nearest(ctx, hs, rep)[:2])))
    ctx.set_mirror_pass(False)
    call("mirror off k9 get_close", get_close(trn, hs, None, 2, m=60))
    call("mirror off k9 raw", raw(hs, rep, 9))
    call("mirror off k9 slow compute", compute(slow, hs, None, 11, m=60), div=True)
    call("mirror off k9 slow get_close", get_close(trn_slow, hs, rep, 12), div=True)
    call("mirror off k9 groups", raw(hs, rep, 13, mask=api.FEAT_FAST | groups))
    ctx.set_mirror_pass(True)
    hs.close()

    # ---- sparse: 16-bit k = 9; 60 x 1 kb alone (lists short enough for the whole-list kernel), then with 24 x 12 kb
    sp = api.HistogramSet(ctx, 9, 16, 60, sparse_entries=sum(len(s) for s in seqs9) + 1024)
    sp.build(seqs9)
    for i in range(4):          # twice the whole-list kernel, then the rank lists are there
        call("sparse short k9 get_close %d" % (i + 1), get_close(trn, sp, None, i, m=60))
    call("sparse short k9 raw", raw(sp, rep, 9))
    call("sparse short k9 slow compute", compute(slow, sp, None, 11, m=60), div=True)
    sp.close()
    sq = list(seqs9) + list(long9)
    sp = api.HistogramSet(ctx, 9, 16, len(sq), sparse_entries=sum(len(s) for s in sq) + 1024)
    sp.build(sq)
    short = np.arange(60, dtype=np.uint32)
    call("sparse k9 short query", get_close(trn, sp, short, 0))                       # (the set's longest list decides: the chunked merge kernel)
    call("sparse k9 parts", raw(sp, None, 61, m=84))                                 # 12 kb lists: a candidate over several waves
    call("sparse k9 ranks 1xm", get_close(trn, sp, short, 1))                        # the third request: rank lists
    call("sparse k9 ranks items", raw(sp, None, 62, m=84))
    call("sparse k9 ranks items window", get_close(api.Trainer(ctx, fast, 0.8), sp, None, 63, m=84))
    call("sparse k9 compute", compute(fast, sp, None, 5, m=84))
    with env("MSC_NO_RANKS_1XM"):
        call("sparse k9 no ranks short", get_close(trn, sp, short, 2))
        call("sparse k9 no ranks parts", raw(sp, None, 64, m=84))
    call("sparse k9 slow compute", compute(slow, sp, None, 6, m=84), div=True)
    call("sparse k9 slow compute long", compute(slow, sp, None, 65, m=84), div=True)
    with env("MSC_RANKS_DIV"):
        call("sparse k9 slow ranks div", compute(slow, sp, None, 6, m=84), div=True)
        call("sparse k9 slow ranks div long", get_close(trn_slow, sp, None, 66, m=84), div=True)
        with env("MSC_NO_RANKS_DIV"):
            call("sparse k9 slow both switches", compute(slow, sp, None, 6, m=84), div=True)
    with env("MSC_NO_RANKS_DIV"):
        call("sparse k9 slow no ranks div", compute(slow, sp, None, 6, m=84), div=True)
    call("sparse k9 groups", raw(sp, rep, 13, mask=api.FEAT_FAST | groups))
    call("sparse k9 filter", lambda: dict(keep=trn.filter(sp, 4, sp, rep)))
    call("sparse k9 merge", lambda: dict(best=np.int64(trn.merge(sp, None, 10, 11, 30, n=60))))
    call("sparse k9 mean_nearest", lambda: dict(zip(("pos", "dist"), api.mean_nearest(ctx, sp, rep)[:2])))
    call("sparse k9 m0", get_close(trn, sp, None, 0, m=0))
    sp.close()
    # ... and the window call on a fresh set: its rank lists are built at the first pass (eager), the close pass rides in the fused
    # epilogue + reduce kernel and the host folds the parts
    for name, t, div in (("fast", trn, False), ("slow", trn_slow, True)):
        sp = api.HistogramSet(ctx, 9, 16, len(sq), sparse_entries=sum(len(s) for s in sq) + 1024)
        sp.build(sq)
        win = api.Window(ctx, sp, np.arange(len(sq) - 1, -1, -1, dtype=np.uint32))
        call("window %s 1" % name, window(win, t, 0, len(sq), sp, 3), div=div)
        win.kill(np.array([30, 31, 40], dtype=np.uint32))
        call("window %s 2" % name, window(win, t, 20, 80, sp, 9), div=div)
        call("window %s long query" % name, window(win, t, 0, 30, sp, 70), div=div)
        win.close()
        sp.close()

    # ---- sparse, generic kernel: a count >= 2^16 in a 32-bit set; a 64-bit k = 13 set
    mono = seqs9[2][:500] + b"A" * 70000 + seqs9[2][500:]
    sq = list(seqs9[:12]) + [mono]
    sp = api.HistogramSet(ctx, 9, 32, len(sq), sparse_entries=sum(len(s) for s in sq) + 1024)
    sp.build(sq)
    for i in range(3):
        call("generic k9 get_close %d" % (i + 1), get_close(api.Trainer(ctx, fast, 0.01), sp, None, 12 if i == 1 else i, m=13))
    call("generic k9 raw", raw(sp, np.array([12, 3, 12, 0], dtype=np.uint32), 12))
    call("generic k9 slow compute", compute(slow, sp, None, 12, m=13), div=True)
    sp.close()
    seqs13, _ = synth.families(6104, 20, 2000, family=5, length_jitter=100)
    sp = api.HistogramSet(ctx, 13, 64, len(seqs13), sparse_entries=sum(len(s) for s in seqs13) + 1024)
    sp.build(seqs13)
    f13 = model(fast9, 13)
    for i in range(3):
        call("sparse u64 k13 get_close %d" % (i + 1), get_close(api.Trainer(ctx, f13, 0.9), sp, None, i, m=20))
    call("sparse u64 k13 raw", raw(sp, np.array([19, 3, 3, 0], dtype=np.uint32), 4))
    call("sparse u64 k13 slow compute", compute(model(slow9, 13), sp, None, 5, m=20), div=True)
    sp.close()

    # ---- two chunks: the second holds one candidate
    seqs7, _ = synth.families(6105, 8, 300, family=4)
    hs = api.HistogramSet(ctx, 7, 32, len(seqs7))
    hs.build(seqs7)
    ctx.set_mirror_pass(False)
    slots = ((np.arange(CHUNK_K7_U32 + 1, dtype=np.uint64) * 5) % 8).astype(np.uint32)
    slots[-1] = 3
    call("two chunks k7 raw", raw(hs, slots, 1))
    call("two chunks k7 compute", compute(model(fast9, 7), hs, slots, 2))
    ctx.set_mirror_pass(True)
    hs.close()

    # ---- the window call over a small dense set (16-bit k = 5: the streaming kernel): 9 000 positions that name 40 slots over and over, the
    # multi-block compaction, the fused epilogue + reduce kernel and -- MSC_NO_FUSED_REDUCE -- epilogue, keyed reduce and k_window_close
    hs = api.HistogramSet(ctx, 5, 16, len(seqs6))
    hs.build(seqs6)
    trn5 = api.Trainer(ctx, api.Feature.from_text(ctx, open(os.path.join(GOLDEN, "weights_k5_u16.txt")).read(), 0), 0.9)
    order = ((np.arange(9000, dtype=np.uint64) * 7919) % 40).astype(np.uint32)
    win = api.Window(ctx, hs, order)
    call("window get_close", window(win, trn5, 100, 8900, hs, 3))
    win.close()
    win = api.Window(ctx, hs, order)
    with env("MSC_NO_FUSED_REDUCE"):
        call("window get_close unfused", window(win, trn5, 100, 8900, hs, 3))
    win.close()
    hs.close()
    ctx.close()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
