#!/usr/bin/env python3
"""msc_set_sparse_matrix_pass: what the matrix-core Q x M pass costs on a SPARSE set next to a dense set of the same sequences -- run on the
GPU box.
    python tools/sparse_matrix_time.py [n_q] [m] [reps] [rate|build]
k = 9 / uint32_t, 1 kb family sequences (synth, families of 20), the model tests/golden/weights_k9_u32.txt; one step = n_q queries against all
m candidates, close flags only (bench.py's step), blocks of 1 024 queries into page-locked flags.
  build   both sets and ONE two-query call on each, which builds their mirrors: the run to put under `rocprofv3 --kernel-trace --stats` for
          the builders' kernel times (sparse: k_kb_build_sparse, k_mb_build_sparse, k_kb_sort, k_ranks_build_sparse, k_ranks16_build;
          dense: k_kb_build, k_kb_sort, k_ranks_build, k_ranks16_build). Prints the calls' wall clock and the device memory each set holds
          before and after its mirrors (hipMemGetInfo differences).
  rate    the same, then the three forms in turn, `reps` times round robin in this one process: dense set; sparse set, switch on; sparse
          set, switch off (one 1 x M pass per query). Device-synchronised wall clock. One JSON line per form.
Nothing here is faster by construction: the figures say what the card did (profiles/sparse_matrix.md)."""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from meshclust2_amd import api, synth

n_q = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
m = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
mode = sys.argv[4] if len(sys.argv) > 4 else "rate"
blk = 1024
ctx = api.Context(0)


def _hip():
    """the HIP runtime the product library has already loaded"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


hip = _hip()


def used_bytes():
    ctx.synchronize()
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


codes, _ = synth.family_codes(2026, m, 1000, family=20)
feat = api.Feature.from_file(ctx, os.path.join(ROOT, "tests", "golden", "weights_k9_u32.txt"), 0)
sets, mem = {}, {}
for name in ("sparse", "dense"):
    before = used_bytes()
    hs = api.HistogramSet(ctx, 9, 32, m, sparse_entries=sum(len(c) for c in codes) + 1024 if name == "sparse" else 0)
    for off in range(0, m, 8192):
        b = synth.pack_batch(codes[off:off + 8192])
        hs.build_packed(off, len(codes[off:off + 8192]), b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"])
    sets[name] = hs
    mem[name] = {"set_bytes": used_bytes() - before}
ctx.set_sparse_matrix_pass(True)
for name in ("sparse", "dense"):          # the first call that takes the route builds the mirrors
    before = used_bytes()
    t0 = time.perf_counter()
    api.score_multi(ctx, feat, sets[name], None, sets[name], np.array([0, 1], dtype=np.uint32), m=m, want=("close",))
    ctx.synchronize()
    mem[name].update(first_call_s=round(time.perf_counter() - t0, 4), mirror_and_scratch_bytes=used_bytes() - before, kernel=ctx.last_kernel_info()[0],
                     reported_bytes=int(sets[name].nbytes()))
    print(json.dumps(dict(mem[name], set=name, m=m, k=9, dtype=32)), flush=True)
if mode == "build":
    sys.exit(0)

q = np.linspace(0, m - 1, n_q).astype(np.uint32)
close = api.pinned_array(ctx, (blk, m), np.uint8)
forms = (("dense", "dense", True), ("sparse_on", "sparse", True), ("sparse_off", "sparse", False))
kernels = {}


def step(which, on):
    ctx.set_sparse_matrix_pass(on)
    hs = sets[which]
    for b0 in range(0, n_q, blk):
        api.score_multi(ctx, feat, hs, None, hs, q[b0:b0 + blk], m=m, want=("close",), out={"close": close[:min(blk, n_q - b0)]})
    ctx.synchronize()


times = {f[0]: [] for f in forms}
for name, which, on in forms:          # warm-up: scratch, page-locked arrays
    step(which, on)
    kernels[name] = ctx.last_kernel_info()[0]
for _ in range(reps):
    for name, which, on in forms:
        t0 = time.perf_counter()
        step(which, on)
        times[name].append(time.perf_counter() - t0)
for name, _, _ in forms:
    t = times[name]
    s = float(np.median(t))
    print(json.dumps({"form": name, "n_q": n_q, "m": m, "k": 9, "dtype": 32, "step_s": round(s, 5), "steps_s": [round(x, 5) for x in t],
                      "pairs_per_s": round(n_q * m / s / 1e9, 3), "spread": round((max(t) - min(t)) / s, 4), "unit": "G pairs/s", "kernel": kernels[name]}), flush=True)
