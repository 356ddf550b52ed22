#!/usr/bin/env python3
"""msc_search_pairs with a --feat slow model: the fallback route against the matrix-core route with the divergence sums from cells
(msc_set_pairs_div_cells) -- run on the GPU box.
    python tools/bench_pairs_div.py [n_q] [m] [reps] [off,on] [--profile DIR]
k = 9 / uint8_t, 1 kb family sequences (synth, families of 20), tests/golden/weights_cfg5_k9.txt (a classification block: jensen_shannon and
four fast statistics). One step = search_pairs of n_q queries (default 1 024) against m candidates (default 100 000), with the switch off
(the route of every release so far: the baseline) and on, in the same process over the same set. Device-synchronised wall clock, one warm-up
step per form, the median of `reps` (>= 5 for a figure that is kept). One JSON line per form, then one with the ratio and whether the two
forms listed the same pairs.
--profile DIR: afterwards one step of the switch-on form in a child process under `rocprofv3 --kernel-trace --stats` (output under DIR); the
kernels' shares of the GPU time and their time per launch (= per block of 128 queries x one chunk of candidates) as a last JSON line.
Nothing here is faster by construction: if the switch-on form is not faster at this shape, the figures say so (profiles/pairs_div_cells.md)."""
import csv, glob, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

argv = sys.argv[1:]
profile_dir = None
if "--profile" in argv:
    i = argv.index("--profile")
    profile_dir = argv[i + 1]
    del argv[i:i + 2]
n_q = int(argv[0]) if len(argv) > 0 else 1024
m = int(argv[1]) if len(argv) > 1 else 100000
reps = int(argv[2]) if len(argv) > 2 else 5
forms = argv[3].split(",") if len(argv) > 3 else ["off", "on"]

if reps > 0:
    import numpy as np
    from meshclust2_amd import api, synth
    ctx = api.Context(0)
    codes, _ = synth.family_codes(2026, m, 1000, family=20)
    hs = api.HistogramSet(ctx, 9, 8, m)
    for off in range(0, m, 8192):
        b = synth.pack_batch(codes[off:off + 8192])
        hs.build_packed(off, len(codes[off:off + 8192]), b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"])
    pred = api.Predictor.from_file(ctx, os.path.join(ROOT, "tests", "golden", "weights_cfg5_k9.txt"))
    q = np.linspace(0, m - 1, n_q).astype(np.uint32)
    rows, lists = {}, {}
    for name in forms:
        ctx.set_pairs_div_cells(name == "on")
        got = pred.search_pairs(hs, None, hs, q, m=m)          # warm-up: mirrors, scratch
        ctx.synchronize()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = pred.search_pairs(hs, None, hs, q, m=m)
            ctx.synchronize()
            t.append(time.perf_counter() - t0)
        s = float(np.median(t))
        info = got[3]
        rows[name] = {"form": "div_cells_" + name, "n_q": n_q, "m": m, "k": 9, "dtype": 8, "model": "weights_cfg5_k9.txt", "step_s": round(s, 5),
                      "steps_s": [round(x, 5) for x in t], "pairs_per_s": round(n_q * m / s / 1e6, 1), "unit": "M pairs/s", "route": info["route"],
                      "n_pairs": info["n_pairs"], "fp64_pairs": info["fp64_pairs"], "kernel": ctx.last_kernel_info()[0]}
        lists[name] = (got[0], got[1])
        print(json.dumps(rows[name]), flush=True)
    ctx.set_pairs_div_cells(False)
    if "off" in rows and "on" in rows:
        same = bool(np.array_equal(lists["off"][0], lists["on"][0]) and np.array_equal(lists["off"][1], lists["on"][1]))
        print(json.dumps({"on_over_off": round(rows["off"]["step_s"] / rows["on"]["step_s"], 3), "same_pairs_listed": same}), flush=True)

if profile_dir:
    os.makedirs(profile_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", profile_dir, "-o", "pairs_div", "--", sys.executable, os.path.abspath(__file__), str(n_q), str(m), "1", "on"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        sys.stdout.write(r.stdout.decode(errors="replace")[-3000:])
        sys.exit(r.returncode)
    found = sorted(glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        sys.exit("no kernel_stats.csv under " + profile_dir)
    kernels = []
    for row in csv.DictReader(open(found[-1])):
        name = row.get("Name", "")
        calls, total = int(row.get("Calls", 0)), float(row.get("TotalDurationNs", 0))
        kernels.append({"kernel": name[:90], "calls": calls, "total_ms": round(total / 1e6, 3), "us_per_launch": round(total / 1e3 / max(calls, 1), 1),
                        "share": float(row.get("Percentage", 0))})
    kernels.sort(key=lambda k: -k["total_ms"])
    print(json.dumps({"kernel_trace": found[-1], "steps_traced": 2, "kernels": kernels[:12]}), flush=True)
