"""Helper run as a subprocess by tests/test_gpu_multi_chunks.py, one process per set of route switches (the library reads them once per
process): msc_score_multi with a block's candidates in SEVERAL chunks, route by route, held to the same call over the distinct slots in
one chunk (gathered by the slot list), which is itself held to the CPU oracle on sampled pairs.

    python multi_chunk_check.py MODE          prints MULTI_CHUNK_OK MODE when every case of the mode held

How many chunks a block must run in is restated here from the caps of msc_api_multi.hip and the three lines of msc_cand_chunks
(msc_multi_plan.h) -- never read from the library -- and every case asserts it through msc_last_kernel_launches (one per chunk, summed over
the call's blocks), so none can pass while running in one chunk."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from meshclust2_amd import api, synth  # noqa: E402
from oracle import oracle_py  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from golden_util import EXACT, FEATS, weights_text  # noqa: E402

# the switches each mode needs; the parent starts the child with these and no other MSC_* variable
MODE_ENV = {
    "matrix": {"MSC_GEMM_SLICES": "64"},
    "contig": {"MSC_GEMM_SLICES": "64"},
    "contig_tiles": {"MSC_MULTI_NO_DIGEST": "1"},
    "digest": {"MSC_MULTI_NO_GEMM": "1"},
    "digest_prefix": {"MSC_MULTI_NO_GEMM": "1", "MSC_MULTI_NO_RANKS": "1"},
    "ring": {"MSC_MULTI_NO_DIGEST": "1"},
    "tiles": {"MSC_MULTI_NO_DIGEST": "1"},
    "groups": {},
}

SEED, N, LEN, K = 20260002, 800, 1000, 9          # the world of tests/test_gpu_emd_bounds.py
NAME_OF_BIT = {bit: name for name, bit in FEATS}
NAME_OF_BIT.update({14: "rre_k_r", 16: "sim_mm"})
FAST_MASK = sum(1 << b for n, b in FEATS if n not in ("jefferey_divergence", "jensen_shannon"))
DIV_BITS, GRP_BITS = (7, 29), (14, 16)
DIV_MASK = (1 << 2) | (1 << 7) | (1 << 29)          # manhattan beside the two divergence sums
GRP_MASK = (1 << 14) | (1 << 16)
ORDERS = (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST)
GEMM, TILES, RING, DIGEST = "k_pair_gemm_fp4_dma<", "k_pair_tiles_multi", "k_pair_tiles_multi32_ring", "k_pair_digest_multi<u8 counts"
# the oracle tolerances tests/test_gpu_parity.py holds the same kernels to: (rel, abs)
TOL_DIV, TOL_GRP, TOL_SUM, TOL_APPROX = (1e-9, 1e-14), (1e-9, 1e-13), (1e-8, 1e-10), (1e-9, 1e-13)

G1_STYLE = """k: %d
mode: 1
max_features: 4
ID: 0.9
Datatype: uint%d_t
feature_set: 81920

n_combos: 3
-0.4
0 65536 1.7
1 81920 -0.9
3 16384 0.35

n_singles: 2
65536 0 0.02
16384 0 0.5
"""


# ---- the chunk arithmetic, restated
def cand_chunks(m, cap):
    """msc_cand_chunks -> (candidates per chunk, chunks)"""
    c0 = min(max(cap, 256), m)
    n = (m + c0 - 1) // c0
    return (m + n - 1) // n, n


def matrix_cap(nq, slices=64):
    """product array [slices][chunk][rows] int32 within 2 GiB; rows: 32, 64 or 128 query rows a block"""
    rows = 32 if nq <= 32 else 64 if nq <= 64 else 128
    return (2048 << 20) // (slices * rows * 4)


def group_cap(nq):
    """[n_q][chunk][16][2] doubles within 1 GiB"""
    return (1024 << 20) // (nq * 32 * 8)


def streamed_cap(route, nq, dtype, k=K, tps=2):
    """partial records of one launch within 4 GiB. digest: 16-byte records, 4^k / 1024 / tps a pair, queries padded to 16; ring: 16-byte
    records, one per 4 KiB tile of the histogram, queries padded to the group of 8 (16 queries and more of 32-bit bins); raw tiles: 24-byte
    records, one per 4 KiB tile"""
    tiles = 4 ** k * (dtype // 8) // 4096
    if route == "digest":
        return (4096 << 20) // ((4 ** k // 1024 // tps) * 16 * ((nq + 15) // 16 * 16))
    if route == "ring":
        return (4096 << 20) // (tiles * 16 * ((nq + 7) // 8 * 8))
    return (4096 << 20) // (tiles * 24 * nq)


def chunks_of_call(n_q, m, block, cap_of):
    """-> [(queries, candidates per chunk, chunks)] per block of the call"""
    return [(min(block, n_q - q0),) + cand_chunks(m, cap_of(min(block, n_q - q0))) for q0 in range(0, n_q, block)]


def launches(plan):
    return sum(n for _, _, n in plan)


# ---- comparisons
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def close_to(got, exp, tol):
    return np.abs(got - exp) <= tol[1] + tol[0] * np.abs(exp)


def draw_slots(n, m):
    """m slots of n, repeats and known values on both sides of every chunk border: the last 64 are the first 64 slots in reverse"""
    slots = np.random.default_rng(5).integers(0, n, size=m).astype(np.uint32)
    slots[-64:] = np.arange(63, -1, -1, dtype=np.uint32)
    return slots


def gathered(plain, slots):
    return {key: (None if v is None else v if key == "counts" else np.ascontiguousarray(v[:, slots])) for key, v in plain.items()}


def tiled(plain, times):
    return {key: (None if v is None else v if key == "counts" else np.concatenate([v] * times, axis=1)) for key, v in plain.items()}


def mask_bits(mask):
    return [b for b in range(64) if mask >> b & 1]


def hold_chunked(tag, got, exp, mask=0, approx_model=False, grp_bits_equal=True):
    """the chunked call against the one-chunk call's values for the same pairs: everything bit for bit but the two divergence columns (the
    merge kernel's parts depend on a launch's candidates) and, with approx_model, the sums of a model that holds them -- those to the oracle
    tolerances, the flags equal except where |sum| is within that tolerance of 0 (at most 10 a call, counted and printed)"""
    own = got["close"].sum(axis=1, dtype=np.uint64) if got["close"] is not None else None
    if got["counts"] is not None:
        assert np.array_equal(got["counts"], own), (tag, "counts != close.sum(axis=1)")
    if got["raw"] is not None:
        for j, b in enumerate(mask_bits(mask)):
            g, e = got["raw"][..., j], exp["raw"][..., j]
            if b in DIV_BITS:
                ok = close_to(g, e, TOL_DIV)
                assert ok.all(), (tag, NAME_OF_BIT[b], int((~ok).sum()), float(np.max(np.abs(g - e))))
            elif b in GRP_BITS and not grp_bits_equal:
                ok = close_to(g, e, TOL_GRP)
                assert ok.all(), (tag, NAME_OF_BIT[b], int((~ok).sum()), float(np.max(np.abs(g - e))))
            else:
                same = bits(g) == bits(e)
                assert same.all(), (tag, NAME_OF_BIT[b], int((~same).sum()), np.argwhere(~same)[:4].tolist())
    for key in ("sum", "csum"):
        if got[key] is None:
            continue
        if approx_model:
            ok = close_to(got[key], exp[key], TOL_SUM)
            assert ok.all(), (tag, key, int((~ok).sum()), float(np.max(np.abs(got[key] - exp[key]))))
        else:
            same = bits(got[key]) == bits(exp[key])
            assert same.all(), (tag, key, int((~same).sum()), np.argwhere(~same)[:4].tolist())
    if got["close"] is not None:
        differ = got["close"] != exp["close"]
        if approx_model:
            near = np.abs(exp["sum"]) <= TOL_SUM[1] + TOL_SUM[0] * np.abs(exp["sum"])
            print("%s: flags that differ beside a sum within tolerance of 0: %d" % (tag, int(differ.sum())))
            assert not (differ & ~near).any() and int(differ.sum()) <= 10, (tag, int(differ.sum()), int((differ & ~near).sum()))
        else:
            assert not differ.any(), (tag, "close", int(differ.sum()), np.argwhere(differ)[:4].tolist())
            if got["counts"] is not None:
                assert np.array_equal(got["counts"], exp["close"].sum(axis=1, dtype=np.uint64)), (tag, "counts")


class World:
    """sequences, the sets built from them per (k, bin type), and the oracle's histograms of the sampled slots"""

    def __init__(self, ctx, seqs):
        self.ctx, self.seqs, self.sets, self.oh, self.oracle_values = ctx, seqs, {}, {}, {}

    def set(self, dtype, k=K):
        if (dtype, k) not in self.sets:
            hs = api.HistogramSet(self.ctx, k, dtype, len(self.seqs))
            for off in range(0, len(self.seqs), 256):
                hs.build(self.seqs[off:off + 256], first_slot=off)
            self.sets[(dtype, k)] = hs
        return self.sets[(dtype, k)]

    def hist(self, dtype, i, k=K):
        if (dtype, k, i) not in self.oh:
            self.oh[(dtype, k, i)] = oracle_py.hist(self.seqs[i], k, dtype)
        return self.oh[(dtype, k, i)]


def oracle_rows(n_q, block):
    """the first query, the last of the full block, the last of the call"""
    return sorted({0, min(block, n_q) - 1, n_q - 1})


def tie_to_oracle(tag, world, dtype, plain, qs, order, mask=0, text=None, block=128, k=K):
    """the one-chunk call, directly against the CPU oracle: three query rows x 200 distinct candidates"""
    n = plain["close"].shape[1] if plain["close"] is not None else plain["raw"].shape[1]
    sample = np.sort(np.random.default_rng(7).choice(n, size=200, replace=False))
    model = oracle_py.predictor(text) if text is not None else None
    cols = mask_bits(mask) if plain["raw"] is not None else []
    rows = oracle_rows(len(qs), block)
    for i in sorted({int(qs[r]) for r in rows} | {int(c) for c in sample}):
        world.hist(dtype, i, k)

    def pair(rc):
        """the oracle's values of one pair (kept per process: calls of one child share query rows) -> (raw statistics, weighted sum)"""
        r, c = rc
        key = (dtype, k, int(qs[r]), int(c), order, mask if cols else 0, text)
        if key not in world.oracle_values:
            hq, hc = world.hist(dtype, int(qs[r]), k), world.hist(dtype, int(c), k)
            a, b = (hc, hq) if order == api.ORDER_CAND_FIRST else (hq, hc)
            world.oracle_values[key] = ([oracle_py.raw_feature(1 << bit, a, b) for bit in cols], oracle_py.score(model.cls, a, b)[2] if model is not None else None)
        return world.oracle_values[key]
    pairs = [(r, int(c)) for r in rows for c in sample]
    with ThreadPoolExecutor(max_workers=16) as pool:          # (the oracle is plain C behind ctypes: its calls run beside one another)
        values = list(pool.map(pair, pairs))
    for (r, c), (raw, wsum) in zip(pairs, values):
        for j, bit in enumerate(cols):
            exp, got, name = raw[j], plain["raw"][r, c, j], NAME_OF_BIT[bit]
            if name in EXACT and name != "kulczynski2":
                assert got == exp, (tag, name, r, c, got, exp)
            else:
                tol = TOL_DIV if bit in DIV_BITS else TOL_GRP if bit in GRP_BITS else TOL_APPROX
                assert abs(got - exp) <= tol[1] + tol[0] * abs(exp), (tag, name, r, c, got, exp)
        if model is not None:
            if plain["sum"] is not None:
                assert abs(plain["sum"][r, c] - wsum) <= TOL_SUM[1] + TOL_SUM[0] * abs(wsum), (tag, "sum", r, c, plain["sum"][r, c], wsum)
            if plain["close"] is not None:
                assert plain["close"][r, c] == (1 if wsum >= 0 else 0), (tag, "close", r, c, wsum)


def emd_text(dtype):
    """weights_k9_u32.txt for a set of `dtype` bins, as tests/test_gpu_emd_bounds.py rewrites it (_text)"""
    text = weights_text("weights_k9_u32.txt").replace("uint32_t", "uint%d_t" % dtype)
    wrapped = "268435456 6.13962398729182e-05 6.19221396338429e-05"
    assert text.count(wrapped) == 1
    return text if dtype == 32 else text.replace(wrapped, "268435456 0.9997 1")


def shifted(text, by):
    """a weights file with the intercept of its classification block lowered by `by` (tests/test_gpu_emd_bounds.py: _shifted, _w0)"""
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("n_combos:")) + 1
    lines[at] = repr(float(lines[at]) - float(by))
    return "\n".join(lines) + "\n"


class Clock:
    def __init__(self):
        self.t = time.time()

    def lap(self, what):
        now = time.time()
        print("  [%.1f s] %s" % (now - self.t, what), flush=True)
        self.t = now


def call(ctx, name, want_launches, *args, **kw):
    """score_multi, the route's kernel name and the launches (= chunks over the call's blocks) asserted -> result"""
    got = api.score_multi(ctx, *args, **kw)
    kernel, n = ctx.last_kernel_info()[0], ctx.last_kernel_launches()
    ok = kernel == name if name in (TILES, RING) else kernel.startswith(name)
    assert ok, (kernel, name)
    assert want_launches is None or n == want_launches, ("launches", n, want_launches, kernel)          # (None: the caller asserts them)
    return got


def blocks_of(n_q, block):
    return (n_q + block - 1) // block


# ---- A: the matrix cores over a slot list, MSC_GEMM_SLICES=64
def mode_matrix(ctx):
    clock = Clock()
    world = World(ctx, synth.families(SEED, N, LEN)[0])
    nq, m = 130, 70000
    qs = np.arange(nq, dtype=np.uint32)
    plan = chunks_of_call(nq, m, 128, matrix_cap)
    assert plan == [(128, 35000, 2), (2, 70000, 1)] and launches(plan) == 3, plan
    slots = draw_slots(N, m)
    hs, text = world.set(32), emd_text(32)
    feat = api.Feature.from_text(ctx, text, 0)
    want = ("sum", "csum", "close", "counts")
    fp64 = {}
    # 1. the scored tail: sums, raw statistics, flags, counts, the rank walk of every pair at the chunk's offset
    for order in ORDERS:
        plain = call(ctx, GEMM, 2, feat, hs, None, hs, qs, order=order, m=N, feat_mask=FAST_MASK, want=want)
        tie_to_oracle("A1 order %d" % order, world, 32, plain, qs, order, FAST_MASK, text)
        got = call(ctx, GEMM, 3, feat, hs, slots, hs, qs, order=order, feat_mask=FAST_MASK, want=want)
        exp = gathered(plain, slots)
        hold_chunked("A1 order %d" % order, got, exp, FAST_MASK)
        fp64[order] = (exp["close"], exp["close"].sum(axis=1, dtype=np.uint64))
        del got, exp, plain
    clock.lap("A1 scored tail, both orders")
    # 2. flags only: the bound screen and the list of open pairs per chunk; a block in several chunks does not fold, no tail group forms
    # The block of 2 runs in ONE chunk, so it may fold, and folded it lists every related pair of its two queries: 2.5 % of a uniform draw
    # against the list's 1.56 %. It then falls back and runs a second time with the true product -- one launch more, which
    # msc_last_fold_screen reports (and the model remembers: a fresh one per call). The block in two chunks must not fold: the call of
    # the first 128 queries alone reports no folded block.
    for order in ORDERS:
        only = call(ctx, GEMM, None, api.Feature.from_text(ctx, text, 0), hs, slots, hs, qs, order=order, want=("close", "counts"))
        n_launches = ctx.last_kernel_launches()
        listed, dense, blocks = ctx.last_emd_walk()
        fold, tgroups = ctx.last_fold_screen(), ctx.last_tail_groups()
        print("A2 order %d: listed %d of %d pairs (%.4f), dense %d of %d chunks, launches %d, fold %r, tail groups %r" % (order, listed, nq * m, listed / (nq * m), dense, blocks, n_launches, fold, tgroups))
        assert np.array_equal(only["close"], fp64[order][0]) and np.array_equal(only["counts"], fp64[order][1]), ("A2", order)
        assert fold[1] <= 1 and fold[2] <= fold[1] and tgroups == (0, 0), (fold, tgroups)          # (only the block of 2 may fold)
        assert n_launches == 3 + fold[2], (n_launches, fold)
        # the walk counters count a block once per chunk: 2 chunks of the block of 128 and the block of 2
        assert blocks == 3 and dense == 0 and 0 < listed <= nq * m // 64, (listed, dense, blocks)
        head = call(ctx, GEMM, 2, feat, hs, slots, hs, qs[:128], order=order, want=("close", "counts"))          # the block in two chunks alone
        assert ctx.last_fold_screen()[1] == 0 and ctx.last_tail_groups() == (0, 0) and ctx.last_emd_walk()[1:] == (0, 2), (ctx.last_fold_screen(), ctx.last_emd_walk())
        assert np.array_equal(head["close"], fp64[order][0][:128])
        ctx.set_emd_bounds(False)
        try:
            off = call(ctx, GEMM, 3, feat, hs, slots, hs, qs, order=order, want=("close", "counts"))
            walk = ctx.last_emd_walk()
        finally:
            ctx.set_emd_bounds(True)
        assert np.array_equal(off["close"], only["close"]) and np.array_equal(off["counts"], only["counts"]) and walk == (0, 3, 3), walk
    clock.lap("A2 flags only, both orders")
    # 3. one chunk's list overflows and the other's does not, in either order of the halves: the list's words are cleared between chunks
    q20 = np.tile(np.arange(20, dtype=np.uint32), 7)[:128]
    fam = api.score_multi(ctx, feat, hs, None, hs, np.arange(20, dtype=np.uint32), m=20, want=("sum",))["sum"]
    moved_text = shifted(text, float(np.median(fam)))
    rng = np.random.default_rng(5)
    strangers, relatives = rng.integers(140, N, size=35000).astype(np.uint32), rng.integers(0, 20, size=35000).astype(np.uint32)
    assert chunks_of_call(128, m, 128, matrix_cap) == [(128, 35000, 2)]
    moved = api.Feature.from_text(ctx, moved_text, 0)
    plain = call(ctx, GEMM, 1, moved, hs, None, hs, q20, m=N, want=("sum", "close", "counts"))
    assert np.array_equal(plain["close"], (plain["sum"] >= 0).astype(np.uint8))
    tie_to_oracle("A3", world, 32, plain, q20, api.ORDER_CAND_FIRST, 0, moved_text)
    share = float(plain["close"][:, :20].mean())
    assert 0.3 < share < 0.7, share          # the threshold runs through the same-family pairs
    for halves in ((strangers, relatives), (relatives, strangers)):
        both = np.concatenate(halves)
        exp = gathered(plain, both)
        model = api.Feature.from_text(ctx, moved_text, 0)          # (fresh: overflow is remembered on the model)
        only = call(ctx, GEMM, 2, model, hs, both, hs, q20, want=("close", "counts"))
        listed, dense, blocks = ctx.last_emd_walk()
        print("A3 %s first: listed %d, dense %d of %d chunks, close among same-family pairs %.3f" % ("strangers" if halves[0] is strangers else "relatives", listed, dense, blocks, share))
        assert np.array_equal(only["close"], exp["close"]), "A3 flags"
        assert np.array_equal(only["counts"], exp["close"].sum(axis=1, dtype=np.uint64)) and np.array_equal(only["counts"], only["close"].sum(axis=1, dtype=np.uint64))
        assert (dense, blocks) == (1, 2), (listed, dense, blocks)          # exactly one of the block's two chunks was walked densely
    clock.lap("A3 overflow in one chunk of two")
    # 4. 8-bit bins, a model without the distance: the f32 screen with the scored tail per chunk, nothing for msc_last_emd_walk to count
    hs8, text8 = world.set(8), weights_text("weights_k9_u8.txt")
    feat8 = api.Feature.from_text(ctx, text8, 0)
    plain = call(ctx, GEMM, 2, feat8, hs8, None, hs8, qs, m=N, want=("sum", "close", "counts"))
    assert np.array_equal(plain["close"], (plain["sum"] >= 0).astype(np.uint8))
    tie_to_oracle("A4", world, 8, plain, qs, api.ORDER_CAND_FIRST, 0, text8)
    exp = gathered(plain, slots)
    only = call(ctx, GEMM, 3, feat8, hs8, slots, hs8, qs, want=("close", "counts"))
    assert ctx.last_emd_walk() == (0, 0, 0), ctx.last_emd_walk()
    hold_chunked("A4", dict(only, sum=None, csum=None, raw=None), exp)
    clock.lap("A4 8-bit bins, no distance")


# ---- B: contiguous candidates (cand_slots = None: the chunk's offset reaches the bins, scalars, headers and kb_first)
def contig_world(ctx):
    """an 8-bit k = 9 set of 70 000 slots (18 GB): one batch of 2 000 sequences built 35 times, slot s holds sequence s mod 2 000"""
    codes = [synth.member(5, t // 20, t % 20, synth.template(5, t // 20, 1000)) for t in range(2000)]
    b = synth.pack_batch(codes)
    big = api.HistogramSet(ctx, K, 8, 70000)
    for done in range(0, 70000, 2000):
        big.build_packed(done, 2000, b["packed"], b["n_bases"], b["seg_seq"], b["seg_start"], b["seg_end"], b["eff_len"], b["one_mers"])
    return World(ctx, [synth.to_ascii(c) for c in codes]), big


def mode_contig(ctx):
    clock = Clock()
    world, big = contig_world(ctx)
    clock.lap("the set of 70 000 slots")
    nq, m, text = 130, 70000, emd_text(8)
    qs = np.arange(nq, dtype=np.uint32) * 15          # (slots 0 .. 1 935: the queries are candidates of the one-chunk call too)
    assert launches(chunks_of_call(nq, m, 128, matrix_cap)) == 3
    feat = api.Feature.from_text(ctx, text, 0)
    want = ("sum", "csum", "close", "counts")
    for order in ORDERS:
        plain = call(ctx, GEMM, 2, feat, big, None, big, qs, order=order, m=2000, feat_mask=FAST_MASK, want=want)
        tie_to_oracle("B1 order %d" % order, world, 8, plain, qs, order, FAST_MASK, text)
        got = call(ctx, GEMM, 3, feat, big, None, big, qs, order=order, m=m, feat_mask=FAST_MASK, want=want)
        exp = tiled(plain, 35)
        hold_chunked("B1 order %d" % order, got, exp, FAST_MASK)
        del got
        only = call(ctx, GEMM, 3, feat, big, None, big, qs, order=order, m=m, want=("close", "counts"))
        listed, dense, blocks = ctx.last_emd_walk()
        print("B2 order %d: listed %d of %d pairs (%.4f), dense %d of %d chunks, fold %r" % (order, listed, nq * m, listed / (nq * m), dense, blocks, ctx.last_fold_screen()))
        assert np.array_equal(only["close"], exp["close"]) and np.array_equal(only["counts"], exp["close"].sum(axis=1, dtype=np.uint64)), ("B2", order)
        assert blocks == 3 and dense == 0 and 0 < listed <= nq * m // 64, (listed, dense, blocks)
        assert ctx.last_fold_screen()[1] <= 1 and ctx.last_tail_groups() == (0, 0)
        del only, exp, plain
        clock.lap("B order %d" % order)


def mode_contig_tiles(ctx):
    """the same set on the raw-tile kernel: blocks of 64 + 64 + 2, the blocks of 64 in two chunks of 35 000"""
    clock = Clock()
    world, big = contig_world(ctx)
    clock.lap("the set of 70 000 slots")
    nq, m, text = 130, 70000, emd_text(8)
    qs = np.arange(nq, dtype=np.uint32) * 15
    plan = chunks_of_call(nq, m, 64, lambda q: streamed_cap("tiles", q, 8))
    assert plan == [(64, 35000, 2), (64, 35000, 2), (2, 70000, 1)], plan
    feat = api.Feature.from_text(ctx, text, 0)
    want = ("sum", "csum", "close", "counts")
    plain = call(ctx, TILES, 3, feat, big, None, big, qs, m=2000, feat_mask=FAST_MASK, want=want)
    tie_to_oracle("B tiles", world, 8, plain, qs, api.ORDER_CAND_FIRST, FAST_MASK, text, block=64)
    got = call(ctx, TILES, 5, feat, big, None, big, qs, m=m, feat_mask=FAST_MASK, want=want)
    hold_chunked("B tiles", got, tiled(plain, 35), FAST_MASK)
    clock.lap("B raw tiles")


# ---- C: the streamed routes over a slot list of 40 000
def streamed(ctx, route, dtype, kernel, name_has=None):
    clock = Clock()
    world = World(ctx, synth.families(SEED, N, LEN)[0])
    hs, text, m = world.set(dtype), emd_text(dtype), 40000
    slots = draw_slots(N, m)
    # two tiles per step of the digest kernel while 64 * 32 * count^2 fits 32 bits: no count passes a sequence's k-mers
    tps = 2 if 64 * 32 * (max(len(s) for s in world.seqs) + 1) ** 2 < 1 << 32 else 1
    assert tps == 2

    def cap_of(nq):
        return streamed_cap(route, nq, dtype, tps=tps)
    per_block = {"digest": (20000, 2), "ring": (13334, 3), "tiles": (20000, 2)}[route]
    assert chunks_of_call(80, m, 64, cap_of) == [(64,) + per_block, (16, 40000, 1)], chunks_of_call(80, m, 64, cap_of)
    grp_of = lambda nq: min(cap_of(nq), group_cap(nq))          # noqa: E731  (the group records' cap is the wider one here)
    assert chunks_of_call(80, m, 64, grp_of) == chunks_of_call(80, m, 64, cap_of)
    feat = api.Feature.from_text(ctx, text, 0)
    slow_text = weights_text("weights_cfg5_k9.txt")          # a model that holds the two divergence sums
    slow = api.Feature.from_text(ctx, slow_text, 0)
    want = ("sum", "csum", "close", "counts")
    for nq in (64, 80):
        qs = (np.arange(nq, dtype=np.uint32) * 7) % N
        n_plain, n_chunked = blocks_of(nq, 64), launches(chunks_of_call(nq, m, 64, cap_of))
        assert n_chunked == per_block[1] + (1 if nq == 80 else 0)
        # the integer statistics, sums, flags, counts
        plain = call(ctx, kernel, n_plain, feat, hs, None, hs, qs, m=N, feat_mask=FAST_MASK, want=want)
        if name_has is not None:
            assert name_has in ctx.last_kernel_info()[0], ctx.last_kernel_info()
        tie_to_oracle("C %s fast %d" % (route, nq), world, dtype, plain, qs, api.ORDER_CAND_FIRST, FAST_MASK, text, block=64)
        got = call(ctx, kernel, n_chunked, feat, hs, slots, hs, qs, feat_mask=FAST_MASK, want=want)
        if name_has is not None:
            assert name_has in ctx.last_kernel_info()[0], ctx.last_kernel_info()
        hold_chunked("C %s fast %d" % (route, nq), got, gathered(plain, slots), FAST_MASK)
        del got, plain
        clock.lap("%d queries, fast statistics" % nq)
        if nq == 80:
            continue
        # the merge pass per query per chunk, under a model that holds its two sums
        wanted = ("sum", "close", "counts")
        plain = call(ctx, kernel, n_plain, slow, hs, None, hs, qs, m=N, feat_mask=DIV_MASK, want=wanted)
        tie_to_oracle("C %s div" % route, world, dtype, plain, qs, api.ORDER_CAND_FIRST, DIV_MASK, slow_text, block=64)
        got = call(ctx, kernel, n_chunked, slow, hs, slots, hs, qs, feat_mask=DIV_MASK, want=wanted)
        hold_chunked("C %s div" % route, got, gathered(plain, slots), DIV_MASK, approx_model=True)
        del got, plain
        clock.lap("divergence mask")
        # the group pass per query per chunk
        plain = call(ctx, kernel, n_plain, feat, hs, None, hs, qs, m=N, feat_mask=GRP_MASK, want=want)
        tie_to_oracle("C %s groups" % route, world, dtype, plain, qs, api.ORDER_CAND_FIRST, GRP_MASK, text, block=64)
        got = call(ctx, kernel, n_chunked, feat, hs, slots, hs, qs, feat_mask=GRP_MASK, want=want)
        hold_chunked("C %s groups" % route, got, gathered(plain, slots), GRP_MASK)
        del got, plain
        clock.lap("group mask")


# ---- D: the cap of the group records, no switch set
def mode_groups(ctx):
    clock = Clock()
    world = World(ctx, synth.families(SEED, N, LEN)[0])
    m = 40000
    slots = draw_slots(N, m)
    want = ("sum", "csum", "close", "counts")
    for dtype, k in ((8, 9), (16, 7)):
        hs, text = world.set(dtype, k), G1_STYLE % (k, dtype)
        feat = api.Feature.from_text(ctx, text, 0)
        # at most 64 slices of 128 rows: the product's cap is 65 536 candidates or more, the group records' decides
        cap_of = lambda nq: min(matrix_cap(nq), group_cap(nq))          # noqa: E731
        assert chunks_of_call(130, m, 128, cap_of) == [(128, 20000, 2), (2, 40000, 1)]
        for nq in (128, 130):
            qs = (np.arange(nq, dtype=np.uint32) * 7) % N
            plain = call(ctx, GEMM, blocks_of(nq, 128), feat, hs, None, hs, qs, m=N, feat_mask=GRP_MASK, want=want)
            tie_to_oracle("D u%d k%d %d" % (dtype, k, nq), world, dtype, plain, qs, api.ORDER_CAND_FIRST, GRP_MASK, text, k=k)
            got = call(ctx, GEMM, 2 if nq == 128 else 3, feat, hs, slots, hs, qs, feat_mask=GRP_MASK, want=want)
            hold_chunked("D u%d k%d %d" % (dtype, k, nq), got, gathered(plain, slots), GRP_MASK)
            del got, plain
            clock.lap("u%d k = %d, %d queries" % (dtype, k, nq))


MODES = {
    "matrix": mode_matrix,
    "contig": mode_contig,
    "contig_tiles": mode_contig_tiles,
    "digest": lambda ctx: streamed(ctx, "digest", 8, DIGEST, "emd by ranks"),
    "digest_prefix": lambda ctx: streamed(ctx, "digest", 8, DIGEST + ">"),
    "ring": lambda ctx: streamed(ctx, "ring", 32, RING),
    "tiles": lambda ctx: streamed(ctx, "tiles", 16, TILES),
    "groups": mode_groups,
}


def main():
    mode = sys.argv[1]
    env = {k: v for k, v in os.environ.items() if k.startswith("MSC_")}
    assert env == MODE_ENV[mode], (env, MODE_ENV[mode])
    ctx = api.Context(0)
    t0 = time.time()
    MODES[mode](ctx)
    print("MULTI_CHUNK_OK %s (%.1f s)" % (mode, time.time() - t0))


if __name__ == "__main__":
    main()
