#!/usr/bin/env python3
"""msc_search_pairs_top (each query's N best pairs, cut on the device) against msc_search_pairs + fetch of the whole list -- run on the GPU box.
    python tools/bench_pairs_top.py [n_q] [m] [reps] [models] [tops] [window] [--profile DIR]
k = 9 / uint32_t, 1 kb family sequences (synth.family_codes(2026, m, 1000, family=20), as bench.py makes them), two model shapes:
  cr -- tests/golden/weights_k9_u32_fc.txt, a classification + regression model over the whole candidate list;
  r  -- its regression block alone (a `mode: 2` file: every pair of a window is listed) over windows of `window` candidates (default
        10 000) centred on each query's own position, the shape of a length window over a length-sorted database.
One step = n_q queries (default 8 192) against m candidates (default 100 000), list fetched to the host. Per model the uncut call
(form "all": msc_search_pairs, the behaviour of every release so far and therefore the baseline) and msc_search_pairs_top with each N of
`tops` (default 1,10), in the same process over the same set. Device-synchronised wall clock, one warm-up step per form, the median of
`reps` (default 3). One JSON line per form with the pairs listed and the bytes of pairs the call's list and the staging list hold at their
peak (12 bytes per pair; the staging list holds one block of queries: the largest block's uncut pairs), then one line per model with the
ratios and whether the cut equals a numpy selection from the uncut list for a sample of queries.
--profile DIR: afterwards one step of the N = tops[0] form of each model in a child process under `rocprofv3 --kernel-trace --stats`
(a run of its own, output under DIR): the kernels' time per launch and share, the two selection kernels next to the product.
Nothing here is faster by construction: the figures say what the cut costs and what it saves (profiles/pairs_top.md)."""
import csv, glob, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

argv = sys.argv[1:]
profile_dir = None
if "--profile" in argv:
    i = argv.index("--profile")
    profile_dir = argv[i + 1]
    del argv[i:i + 2]
n_q = int(argv[0]) if len(argv) > 0 else 8192
m = int(argv[1]) if len(argv) > 1 else 100000
reps = int(argv[2]) if len(argv) > 2 else 3
models = argv[3].split(",") if len(argv) > 3 else ["cr", "r"]
tops = [int(x) for x in argv[4].split(",")] if len(argv) > 4 else [1, 10]
window = int(argv[5]) if len(argv) > 5 else 10000

if reps > 0:
    import numpy as np
    from meshclust2_amd import api, synth
    from golden_util import weights_text, weights_with_mode
    ctx = api.Context(0)
    codes, _ = synth.family_codes(2026, m, 1000, family=20)
    hs = api.HistogramSet(ctx, 9, 32, m)
    for off in range(0, m, 8192):
        b = synth.pack_batch(codes[off:off + 8192])
        hs.build_packed(off, len(codes[off:off + 8192]), b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"])
    text = weights_text("weights_k9_u32_fc.txt")
    q = np.linspace(0, m - 1, n_q).astype(np.uint32)
    for model in models:
        pred = api.Predictor.from_text(ctx, text if model == "cr" else weights_with_mode(text, 2))
        kw = dict(m=m)
        if model == "r":
            lo = np.clip(q.astype(np.int64) - window // 2, 0, max(m - window, 0)).astype(np.uint64)
            kw.update(win_lo=lo, win_hi=lo + np.uint64(min(window, m)))
        rows, full = {}, None
        for top in [0] + tops:
            fn = (lambda: pred.search_pairs(hs, None, hs, q, **kw)) if top == 0 else (lambda: pred.search_pairs_top(hs, None, hs, q, top, **kw))
            got = fn()          # warm-up: mirrors, scratch, the lists' capacity
            ctx.synchronize()
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                got = fn()
                ctx.synchronize()
                t.append(time.perf_counter() - t0)
            s = float(np.median(t))
            info = got[3]
            if top == 0:
                full = got
            counts = np.diff(full[0]).astype(np.int64)
            per_block = [int(counts[b0:b0 + 128].sum()) for b0 in range(0, n_q, 128)]          # (plan_blocks: 128 queries, give or take the last one)
            rows[top] = {"model": model, "form": "top_%d" % top if top else "all", "n_q": n_q, "m": m, "window": window if model == "r" else None, "k": 9, "dtype": 32,
                         "step_s": round(s, 5), "steps_s": [round(x, 5) for x in t], "route": info["route"], "n_pairs": info["n_pairs"],
                         "uncut_pairs": int(counts.sum()), "fp64_pairs": info["fp64_pairs"], "list_bytes": 12 * info["n_pairs"],
                         "staging_bytes": 12 * max(per_block) if top else 0}
            print(json.dumps(rows[top]), flush=True)
            if top:          # a sample of queries against the numpy selection from the uncut list
                same = True
                for j in range(0, n_q, max(1, n_q // 64)):
                    a, e = int(full[0][j]), int(full[0][j + 1])
                    key = full[2][a:e] + 0.0
                    keep = np.sort(np.lexsort((np.arange(key.size), -key))[:top]) + a
                    ga, ge = int(got[0][j]), int(got[0][j + 1])
                    same = same and np.array_equal(got[1][ga:ge], full[1][keep]) and np.array_equal(got[2][ga:ge].view(np.uint64), full[2][keep].view(np.uint64))
                rows[top]["sample_equals_numpy_selection"] = bool(same)
        print(json.dumps({"model": model, "all_over_top": {str(t): round(rows[0]["step_s"] / rows[t]["step_s"], 3) for t in tops},
                          "sample_equals_numpy_selection": all(rows[t]["sample_equals_numpy_selection"] for t in tops)}), flush=True)
        del full, got

if profile_dir:
    os.makedirs(profile_dir, exist_ok=True)
    for model in models:
        name = "pairs_top_" + model
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", profile_dir, "-o", name, "--", sys.executable, os.path.abspath(__file__), str(n_q), str(m), "1", model,
               str(tops[0]), str(window)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode != 0:
            sys.stdout.write(r.stdout.decode(errors="replace")[-3000:])
            sys.exit(r.returncode)
        found = sorted(glob.glob(os.path.join(profile_dir, "**", name + "*kernel_stats.csv"), recursive=True))
        if not found:
            sys.exit("no kernel_stats.csv under " + profile_dir)
        kernels = []
        for row in csv.DictReader(open(found[-1])):
            calls, total = int(row.get("Calls", 0)), float(row.get("TotalDurationNs", 0))
            kernels.append({"kernel": row.get("Name", "")[:90], "calls": calls, "total_ms": round(total / 1e6, 3), "us_per_launch": round(total / 1e3 / max(calls, 1), 1),
                            "share": float(row.get("Percentage", 0))})
        kernels.sort(key=lambda k: -k["total_ms"])
        top_k = [k for k in kernels if "k_pair_top" in k["kernel"]]
        print(json.dumps({"model": model, "kernel_trace": found[-1], "steps_traced": "2 uncut + 2 cut (a warm-up and a timed step each)", "selection": top_k,
                          "kernels": kernels[:10]}), flush=True)
