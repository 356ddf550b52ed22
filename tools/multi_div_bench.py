#!/usr/bin/env python3
"""msc_score_multi with a --feat slow model: one merge pass per query behind the matrix product (the default) against the divergence sums
from cells in the epilogue (msc_set_multi_div_cells) -- run on the GPU box.
    python tools/multi_div_bench.py [m] [n_q] [reps] [--no-pipe] [--only off|on]
    python tools/multi_div_bench.py [m] [n_q] --profile DIR
The shape of bench.py's slow_model_leg: m (default 100 000) family sequences of 1 kb, k = 9, 32-bit bins, dense; n_q (default 256) queries
(slots (j * 7919 + 11) % m) against all of them; tests/golden/weights_cfg5_k9.txt; want = ("close", "counts"), the flags into pinned memory.
One untimed warm-up call per switch setting (mirrors, scratch), then `reps` (default 5) timed calls per setting, ALTERNATING off / on in one
process over the same set; a host clock around a call that ends in synchronize. One JSON line per setting (median, spread = max - min, every
time, msc_last_kernel_info's name), then one with the ratio and whether the two settings gave the same flags and counts. The switch-off call
is the code path of every release so far: its kernel info names the product kernel WITHOUT "divergence sums from cells" -- the sums then
come from k_pair_sparse_mp passes, one per query, queued behind it (what the per-kernel table shows).
--no-pipe: set_block_pipe(False), every kernel of a block on one stream.
--profile DIR: no timing here; per setting one child process (warm-up + one call, block pipe off) under `rocprofv3 --kernel-trace --stats`,
and the kernels' total time, launches and time per launch as one JSON line per setting.
Nothing here is faster by construction: if switch on is not faster at this shape, the figures say so (profiles/multi_div_cells.md)."""
import csv, glob, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

argv = sys.argv[1:]
profile_dir = only = None
if "--profile" in argv:
    i = argv.index("--profile")
    profile_dir = argv[i + 1]
    del argv[i:i + 2]
if "--only" in argv:
    i = argv.index("--only")
    only = argv[i + 1]
    del argv[i:i + 2]
pipe = "--no-pipe" not in argv
argv = [a for a in argv if a != "--no-pipe"]
m = int(argv[0]) if len(argv) > 0 else 100000
n_q = int(argv[1]) if len(argv) > 1 else 256
reps = int(argv[2]) if len(argv) > 2 else 5

if profile_dir:
    os.makedirs(profile_dir, exist_ok=True)
    for name in ("off", "on"):
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(profile_dir, name), "-o", "multi_div", "--", sys.executable, os.path.abspath(__file__),
               str(m), str(n_q), "1", "--no-pipe", "--only", name]
        try:          # (set build ~15 s, warm-up and one call under a second; the tracer's start and its files on top)
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        except subprocess.TimeoutExpired as e:          # a hang: nothing more is started on the GPU
            sys.stdout.write((e.stdout or b"").decode(errors="replace")[-3000:])
            sys.exit("the traced run with the switch %s did not end within 240 s" % name)
        if r.returncode != 0:
            sys.stdout.write(r.stdout.decode(errors="replace")[-3000:])
            sys.exit(r.returncode)
        found = sorted(glob.glob(os.path.join(profile_dir, name, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            sys.stdout.write(r.stdout.decode(errors="replace")[-2000:])
            sys.exit("no kernel_stats.csv under " + os.path.join(profile_dir, name))
        kernels = []
        for row in csv.DictReader(open(found[-1])):
            calls, total = int(row.get("Calls", 0)), float(row.get("TotalDurationNs", 0))
            kernels.append({"kernel": row.get("Name", "")[:90], "calls": calls, "total_ms": round(total / 1e6, 3), "us_per_launch": round(total / 1e3 / max(calls, 1), 1),
                            "share": float(row.get("Percentage", 0))})
        kernels.sort(key=lambda k: -k["total_ms"])
        print(json.dumps({"switch": name, "kernel_trace": found[-1], "calls_traced": "set build + warm-up + 1", "kernels": kernels[:14]}), flush=True)
    sys.exit(0)

import numpy as np
from meshclust2_amd import api, synth
ctx = api.Context(0)
ctx.set_block_pipe(pipe)
hs = api.HistogramSet(ctx, 9, 32, m)
codes, _ = synth.family_codes(20260002, m, 1000, family=20)          # (bench.py's seed and families of 20)
for off in range(0, m, 8192):
    b = synth.pack_batch(codes[off:off + 8192])
    hs.build_packed(off, len(codes[off:off + 8192]), b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"])
del codes
wtext = open(os.path.join(ROOT, "tests", "golden", "weights_cfg5_k9.txt")).read().replace("uint8_t", "uint32_t")
feat = api.Feature.from_text(ctx, wtext, 0)
qs = np.array([(j * 7919 + 11) % m for j in range(n_q)], dtype=np.uint32)
forms = [only] if only else ["off", "on"]
out = {name: {"close": api.pinned_array(ctx, (n_q, m), np.uint8)} for name in forms}


def call(name):
    ctx.set_multi_div_cells(name == "on")
    t0 = time.perf_counter()
    res = api.score_multi(ctx, feat, hs, None, hs, qs, m=m, want=("close", "counts"), out=out[name])
    ctx.synchronize()
    return time.perf_counter() - t0, res, ctx.last_kernel_info()[0]


times, last, kernel = {name: [] for name in forms}, {}, {}
for name in forms:          # warm-up: mirrors, scratch
    call(name)
for _ in range(reps):
    for name in forms:
        dt, last[name], kernel[name] = call(name)
        times[name].append(dt)
ctx.set_multi_div_cells(False)
med = {}
for name in forms:
    t = times[name]
    med[name] = float(np.median(t))
    print(json.dumps({"switch": name, "n_q": n_q, "m": m, "k": 9, "dtype": 32, "model": "weights_cfg5_k9.txt", "block_pipe": pipe, "call_s_median": round(med[name], 5),
                      "call_s_spread": round(max(t) - min(t), 5), "call_s": [round(x, 5) for x in t], "pairs_per_s": round(n_q * m / med[name] / 1e6, 1), "unit": "M pairs/s",
                      "ms_per_128_queries": round(med[name] / n_q * 128 * 1e3, 3), "close_pairs": int(np.sum(last[name]["counts"])), "kernel": kernel[name],
                      "sparse_mirror_entries_slot0": int(hs.entries(0))}), flush=True)
if len(forms) == 2:
    same = bool(np.array_equal(last["off"]["close"], last["on"]["close"]) and np.array_equal(last["off"]["counts"], last["on"]["counts"]))
    print(json.dumps({"off_over_on": round(med["off"] / med["on"], 3), "same_flags_and_counts": same}), flush=True)
