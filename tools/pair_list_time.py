#!/usr/bin/env python3
"""msc_score_pair_list against what a caller had to write without it -- run on the GPU box.
    python tools/pair_list_time.py [cases] [reps] [--lib PATH] [--length BASES]
k = 9 / uint32_t, 1 kb sequences. One process, device-synchronised wall clock and the HIP-event time of the pass kernel
(msc_last_kernel_ms), one warm-up per form, the median of `reps` (default 5). One JSON line per form. cases (default a,b,c):
  a -- the training shape: 300 templates x 8 mutants (golden_util.training_set), 2 400 pairs (template, mutant) with all-distinct second
       slots, FEAT_FAST raw statistics, on a dense and on a sparse set: ONE msc_score_pair_list call against the loop of one
       msc_pair_features_raw call per distinct second slot (what build_table ran before the call existed); the two tables must be equal.
  b -- 1 000 000 member-to-centre pairs over 100 000 sparse slots (families of 20: the centre is a family's first member), the weighted sum
       of tests/golden/weights_k9_u32.txt per pair. The kernel follows the process's environment: run once as is (k_pair_sparse_wl_pairs) and
       once with MSC_SPARSE_NO_WL=1 (k_pair_sparse_mp<.., PAIRS>); the line names the kernel that ran. --length BASES: sequences of that
       length instead of 1 kb (450: two lists fit the whole-list kernel's rule).
  c -- the wall time of msc_train_class (FEAT_FAST, 4 features) on the pairs of case a, 2 000 training and 400 testing.
--lib PATH loads another build of libmeshclust2_hip.so (a build of the parent commit for the "before" of case c; cases a's list form and b
are skipped when that library has no msc_score_pair_list). Nothing here is faster by construction (profiles/pair_list.md)."""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

argv = sys.argv[1:]
lib_path = None
if "--lib" in argv:
    i = argv.index("--lib")
    lib_path = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
length = 1000
if "--length" in argv:
    i = argv.index("--length")
    length = int(argv[i + 1])
    del argv[i:i + 2]
cases = argv[0].split(",") if len(argv) > 0 else ["a", "b", "c"]
reps = int(argv[1]) if len(argv) > 1 else 5

import numpy as np
from meshclust2_amd import _capi
if lib_path:
    _capi.LIB_PATH = lib_path
    if not hasattr(ctypes.CDLL(lib_path), "msc_score_pair_list"):
        _capi.PROTOTYPES.pop("msc_score_pair_list", None)
from meshclust2_amd import api, synth
from golden_util import training_set, weights_text
HAVE_LIST = "msc_score_pair_list" in _capi.PROTOTYPES
K, DT = 9, 32
ctx = api.Context(0)


def timed(fn):
    """-> (median wall s, median pass-kernel ms, last result)"""
    got = fn()          # warm-up: scratch, mirrors, rank lists
    ctx.synchronize()
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = fn()
        ctx.synchronize()
        wall.append(time.perf_counter() - t0)
        try:
            kern.append(ctx.last_kernel_ms()[0])
        except api.MscError:
            kern.append(float("nan"))
    return float(np.median(wall)), float(np.median(kern)), got


def line(**kw):
    kw.update(k=K, dtype=DT, reps=reps, lib=lib_path or "this tree")
    print(json.dumps(kw), flush=True)


if "a" in cases or "c" in cases:
    seqs, pairs = training_set(20261018, 300, 8, 1000)
    first = np.array([p[0] for p in pairs], dtype=np.uint32)
    second = np.array([p[1] for p in pairs], dtype=np.uint32)
    labels = np.array([p[2] for p in pairs])
    assert len(pairs) == 2400 and np.unique(second).size == 2400
    for layout in ("dense", "sparse"):
        hs = api.HistogramSet(ctx, K, DT, len(seqs), sparse_entries=(sum(len(s) for s in seqs) + 64) if layout == "sparse" else 0)
        hs.build(seqs)
        if "a" in cases:
            def loop():
                out = np.zeros((len(first), 9))
                for i in range(len(first)):          # every second slot is distinct: one call per pair
                    out[i] = api.pair_features_raw(ctx, hs, first[i:i + 1], hs, int(second[i]), api.FEAT_FAST)[0]
                return out
            w, km, table = timed(loop)
            line(case="a", layout=layout, form="loop of msc_pair_features_raw per distinct b", pairs=2400, wall_s=round(w, 5), kernel=ctx.last_kernel_info()[0],
                 last_call_kernel_ms=round(km, 4))
            if HAVE_LIST:
                w2, km2, got = timed(lambda: api.score_pair_list(ctx, None, hs, first, hs, second, api.ORDER_CAND_FIRST, api.FEAT_FAST)["raw"])
                line(case="a", layout=layout, form="one msc_score_pair_list call", pairs=2400, wall_s=round(w2, 5), kernel=ctx.last_kernel_info()[0], pass_kernel_ms=round(km2, 4),
                     equals_loop=bool(np.array_equal(got, table, equal_nan=True)), loop_over_list=round(w / w2, 2))
        if "c" in cases:
            w, _, got = timed(lambda: api.train_class(ctx, hs, first, second, labels, 2000, api.FEAT_FAST, 4, 4, 0.8))
            line(case="c", layout=layout, form="msc_train_class", pairs=2400, wall_s=round(w, 5), train_acc=got[1], test_acc=got[2], text_bytes=len(got[0]))
        hs.close()

if "b" in cases and HAVE_LIST:
    m, n = 100000, 1000000
    codes, _ = synth.family_codes(2026, m, length, family=20)
    hs = api.HistogramSet(ctx, K, DT, m, sparse_entries=sum(c.size for c in codes) + 4096)
    for off in range(0, m, 8192):
        b = synth.pack_batch(codes[off:off + 8192])
        hs.build_packed(off, len(codes[off:off + 8192]), b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"])
    feat = api.Feature.from_text(ctx, weights_text("weights_k9_u32.txt"), 0)
    a = np.random.default_rng(7).integers(0, m, n).astype(np.uint32)
    centre = (a // 20 * 20).astype(np.uint32)
    w, km, got = timed(lambda: api.score_pair_list(ctx, feat, hs, a, hs, centre, api.ORDER_CAND_FIRST, 0, want=("sum",))["sum"])
    name = ctx.last_kernel_info()[0]
    # a sample of rows against the per-pair call
    same = all(got[i] == feat.compute(hs, a[i:i + 1], hs, int(centre[i]))["sum"][0] for i in range(0, n, n // 50))
    line(case="b", layout="sparse", form="one msc_score_pair_list call", pairs=n, slots=m, max_nnz=hs.build_info()[3], wall_s=round(w, 5), kernel=name, length=length,
         pass_kernel_ms=round(km, 4), no_wl=os.environ.get("MSC_SPARSE_NO_WL") is not None, sample_equals_per_pair=bool(same))
ctx.close()
