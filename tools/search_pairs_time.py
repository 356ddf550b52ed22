#!/usr/bin/env python3
"""What a Q x M search costs by how its result comes home -- run on the GPU box.
    python tools/search_pairs_time.py [n_q] [m] [reps] [a,b,c]
k = 9 / uint32_t, 1 kb family sequences (synth, families of 20), the mode-3 model tests/golden/weights_k9_u32_fc.txt. One step = the n_q
queries against all m candidates:
  (a) msc_score_multi, close flags only (bench.py's step), blocks of 1 024 queries into page-locked [1024][m] flags;
  (b) what msc::Predictor::search_block does per block: the same flags call plus the regression call with sum_out ([1024][m] FP64 sums);
  (c) msc_search_pairs over all n_q queries at once, plus msc_search_pairs_fetch of the whole list.
Device-synchronised wall clock, one warm-up step, the median of `reps`. One JSON line per form."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from meshclust2_amd import api, synth

n_q = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
m = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
forms = sys.argv[4].split(",") if len(sys.argv) > 4 else ["a", "b", "c"]
blk = 1024
ctx = api.Context(0)
codes, _ = synth.family_codes(2026, m, 1000, family=20)
hs = api.HistogramSet(ctx, 9, 32, m)
for off in range(0, m, 8192):
    b = synth.pack_batch(codes[off:off + 8192])
    hs.build_packed(off, len(codes[off:off + 8192]), b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"])
pred = api.Predictor.from_file(ctx, os.path.join(ROOT, "tests", "golden", "weights_k9_u32_fc.txt"))
q = np.linspace(0, m - 1, n_q).astype(np.uint32)
close = api.pinned_array(ctx, (blk, m), np.uint8) if ("a" in forms or "b" in forms) else None
sums = api.pinned_array(ctx, (blk, m), np.float64) if "b" in forms else None
lib, h = ctx.lib, ctx.h


def step_a():
    for b0 in range(0, n_q, blk):
        api.score_multi(ctx, pred.cls, hs, None, hs, q[b0:b0 + blk], m=m, want=("close",), out={"close": close[:min(blk, n_q - b0)]})


def step_b():
    for b0 in range(0, n_q, blk):
        nb = min(blk, n_q - b0)
        api.score_multi(ctx, pred.cls, hs, None, hs, q[b0:b0 + blk], m=m, want=("close",), out={"close": close[:nb]})
        api.score_multi(ctx, pred.reg, hs, None, hs, q[b0:b0 + blk], m=m, want=("sum",), out={"sum": sums[:nb]})
        np.clip(sums[:nb], 0.0, 1.0, out=sums[:nb])


info = {}


def step_c():
    info.update(pred.search_pairs(hs, None, hs, q, m=m)[3])


for name, fn in (("a", step_a), ("b", step_b), ("c", step_c)):
    if name not in forms:
        continue
    fn()          # warm-up: mirrors, scratch, page-locked arrays
    ctx.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        t.append(time.perf_counter() - t0)
    s = float(np.median(t))
    row = {"form": name, "n_q": n_q, "m": m, "k": 9, "dtype": 32, "step_s": round(s, 5), "steps_s": [round(x, 5) for x in t],
           "pairs_per_s": round(n_q * m / s / 1e9, 3), "unit": "G pairs/s", "kernel": ctx.last_kernel_info()[0]}
    if name == "c":
        row.update(n_pairs=info["n_pairs"], close_fraction=info["n_pairs"] / float(n_q * m), fp64_pairs=info["fp64_pairs"], route=info["route"])
    print(json.dumps(row), flush=True)
