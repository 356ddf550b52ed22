"""msc_set_sparse_matrix_pass: msc_score_multi and msc_search_pairs over two SPARSE sets on the matrix-core route, the three mirrors (presence
bits, lists of large bins, ranks) built from the sets' entry lists. Every switch-on result is held to the switch-off call (one 1 x M pass per
query over the lists: the parent's code path) bit for bit, and anchored outside the feature: the dense sets' call on the same sequences, the CPU
oracle, and the reference's own fastcar output (tests/golden/fastcar_k9_u32.out)."""
import os
import subprocess

import numpy as np
import pytest

from golden_util import EXACT, FEATS, weights_text
from meshclust2_amd import api, synth

pytestmark = pytest.mark.gpu
GEMM = "k_pair_gemm_fp4_dma<"
SPARSE_KERNELS = ("k_pair_sparse_wl", "k_pair_sparse_mp", "k_pair_sparse_mp+wl", "k_pair_ranks_1xm")          # what a sparse Q x M call names without the switch
FAST_MASK = sum(1 << b for name, b in FEATS if name not in ("jefferey_divergence", "jensen_shannon"))          # the nine non-divergence statistics
RTOL = 1e-9
WANT = ("sum", "csum", "close", "counts")
KEYS = ("raw", "sum", "csum", "close", "counts")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.set_sparse_matrix_pass(False)
    c.set_pairs_div_cells(False)
    c.close()


def _repeat_bearing(seqs, every, kind):
    """the construction of tests/test_gpu_qxm_direct.py: a homopolymer / dinucleotide / 12-mer / 3-mer run spliced into every `every`-th sequence"""
    out = []
    for i, s in enumerate(seqs):
        s = bytes(s)
        if i % every == 1:
            at = 100 + 13 * (i % 50)
            run = {"homo": b"A" * 400, "di": b"AC" * 200, "unit12": b"ACGTTGCAAGTC" * 11, "unit3": b"ACG" * 40}[kind]
            s = s[:at] + run + s[at:]
        out.append(s)
    return out


def _sets(ctx, seqs, k, dtype, capacity=None, extra_entries=0):
    """one sparse and one dense set of the same sequences"""
    cap = capacity or len(seqs)
    sp = api.HistogramSet(ctx, k, dtype, cap, sparse_entries=sum(len(s) for s in seqs) + 1024 + extra_entries)
    de = api.HistogramSet(ctx, k, dtype, cap)
    sp.build(seqs)
    de.build(seqs)
    return sp, de


def _text(k, dtype, name="weights_k9_u32.txt"):
    return weights_text(name).replace("k: 9", "k: %d" % k).replace("uint32_t", "uint%d_t" % dtype)


def _multi(ctx, on, feat, hs, cands, q_slots, **kw):
    """score_multi with the switch set for this call -> (results, kernel name)"""
    ctx.set_sparse_matrix_pass(on)
    try:
        got = api.score_multi(ctx, feat, hs, cands, hs, q_slots, **kw)
        return got, ctx.last_kernel_info()[0]
    finally:
        ctx.set_sparse_matrix_pass(False)


def _same(a, b, where, keys=KEYS):
    for key in keys:
        if a[key] is None and b[key] is None:
            continue
        assert np.array_equal(a[key], b[key]), (key, where)


# ------------------------------------------------------------------------------------------------ A. route and results
@pytest.mark.parametrize("dtype,k,n,length,nq,repeats", [
    (32, 9, 150, 1000, 128, None),            # cfg2's shape, a whole block of queries; 16-bit rank walk
    (32, 9, 150, 1000, 130, "di"),            # two blocks; two counts of ~196
    (16, 9, 90, 1000, 64, "unit12"),          # counts 9 .. 16
    (8, 9, 90, 1000, 20, "homo"),             # ~390 copies of bin 0, saturating at 255: reduced ranks past 16 bits, the 32-bit rank walk
    (16, 8, 80, 2000, 9, "unit3"),            # counts ~40
    (8, 8, 60, 500, 5, None),                 # 64 KiB: the smallest histogram a sparse set may have
    (32, 7, 120, 600, 70, None),              # likewise, 32-bit bins; sub-ranges of 1 024 bins, one window of the builder
    (8, 10, 40, 1000, 33, "homo"),            # 2^20 bins: the largest the route takes, 128 windows per block of slots
])
def test_route_and_results(ctx, oracle, dtype, k, n, length, nq, repeats):
    seqs, _ = synth.families(5200 + 31 * k + dtype + nq, n, length, family=6, length_jitter=length // 10)
    seqs = _repeat_bearing(seqs, 7, repeats) if repeats else [bytes(s) for s in seqs]
    sp, de = _sets(ctx, seqs, k, dtype)
    text = _text(k, dtype)
    feat = api.Feature.from_text(ctx, text, 0)
    pred = oracle.predictor(text)
    rng = np.random.default_rng(k * 1000 + nq)
    q_slots = rng.integers(0, n, nq).astype(np.uint32)
    q_slots[:3] = (1, 8, 0)          # repeat-bearing queries (slots 1, 8), a plain one
    cands = np.concatenate([np.arange(n, dtype=np.uint32), rng.integers(0, n, 9).astype(np.uint32)])
    oh = [oracle.hist(s, k, dtype) for s in seqs]
    fast = [(name, b) for name, b in FEATS if (1 << b) & FAST_MASK]
    for order in (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST):
        kw = dict(order=order, feat_mask=FAST_MASK, want=WANT)
        on, kernel = _multi(ctx, True, feat, sp, cands, q_slots, **kw)
        assert kernel.startswith(GEMM), (kernel, dtype, k, repeats)                    # 1. the route
        off, k_off = _multi(ctx, False, feat, sp, cands, q_slots, **kw)
        assert k_off in SPARSE_KERNELS, k_off
        _same(on, off, ("switch off", order, kernel, k_off))                           # 2. today's route
        dense, k_dense = _multi(ctx, True, feat, de, cands, q_slots, **kw)
        assert k_dense.startswith(GEMM) and "mirrors from lists" not in k_dense, k_dense
        _same(on, dense, ("dense", order, kernel))                                     # 3. the dense sets
        assert np.array_equal(on["counts"], on["close"].sum(axis=1, dtype=np.uint64))
        for qi in list(range(0, nq, max(1, nq // 6))) + [0, 1, 2]:                     # 4. the oracle
            q = int(q_slots[qi])
            for ci in list(range(0, len(cands), 11)) + [1, 8]:
                c = int(cands[ci])
                a, b = (oh[c], oh[q]) if order == api.ORDER_CAND_FIRST else (oh[q], oh[c])
                for col, (name, bit) in enumerate(fast):
                    exp = oracle.raw_feature(1 << bit, a, b)
                    val = on["raw"][qi][ci][col]
                    if name in EXACT and name != "kulczynski2":
                        assert val == exp, (name, q, c, order, kernel)
                    else:
                        assert val == pytest.approx(exp, rel=RTOL, abs=1e-13), (name, q, c, order, kernel)
                if order == api.ORDER_CAND_FIRST:
                    _, _, w = oracle.score(pred.cls, oh[c], oh[q])
                    assert on["sum"][qi][ci] == pytest.approx(w, rel=1e-8, abs=1e-10), (q, c, kernel)
                    assert on["close"][qi][ci] == (1 if round(1.0 / (1.0 + np.exp(-w))) > 0 else 0), (q, c, kernel)
    for h in oh:
        oracle.lib().orc_hist_free(h)


# ------------------------------------------------------------------------------------------------ B. three blocks through the pipe
def test_three_blocks_flags_only(ctx):
    seqs, _ = synth.families(5301, 150, 1000, family=6, length_jitter=100)
    seqs = [bytes(s) for s in seqs]
    sp, _ = _sets(ctx, seqs, 9, 32)
    feat = api.Feature.from_text(ctx, _text(9, 32), 0)
    q_slots = np.random.default_rng(53).integers(0, 150, 300).astype(np.uint32)
    cands = np.arange(150, dtype=np.uint32)
    on, kernel = _multi(ctx, True, feat, sp, cands, q_slots, want=("close", "counts"))          # flags alone: the f32 screen
    assert kernel.startswith(GEMM), kernel
    off, k_off = _multi(ctx, False, feat, sp, cands, q_slots, want=("close", "counts"))
    assert k_off in SPARSE_KERNELS, k_off
    _same(on, off, "three blocks", keys=("close", "counts"))
    assert 0 < int(on["counts"].sum()) < 300 * 150


# ------------------------------------------------------------------------------------------------ C. pitch re-layout
def test_lists_of_large_bins_past_the_first_pitch(ctx):
    rng = np.random.default_rng(54)
    seqs, _ = synth.families(5302, 96, 1000, family=6, length_jitter=100)
    seqs = [bytes(s) for s in seqs]
    for i in range(5, 96, 8):          # a random 40-mer six times over: ~40 bins of count >= 3, past the pitch of 16 the lists start with
        unit = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=40))
        seqs[i] = seqs[i][:300] + unit * 6 + seqs[i][300:]
    sp, de = _sets(ctx, seqs, 9, 32)
    feat = api.Feature.from_text(ctx, _text(9, 32), 0)
    q_slots = np.arange(0, 96, 2, dtype=np.uint32)
    q_slots[:2] = (5, 13)
    cands = np.arange(96, dtype=np.uint32)
    kw = dict(feat_mask=FAST_MASK, want=WANT)
    on, kernel = _multi(ctx, True, feat, sp, cands, q_slots, **kw)
    assert kernel.startswith(GEMM), kernel
    off, _ = _multi(ctx, False, feat, sp, cands, q_slots, **kw)
    dense, k_dense = _multi(ctx, True, feat, de, cands, q_slots, **kw)
    assert k_dense.startswith(GEMM), k_dense
    _same(on, off, "switch off")
    _same(on, dense, "dense")


# ------------------------------------------------------------------------------------------------ D. a declined block
def test_a_block_with_a_long_hot_list_stays_on_the_list_passes(ctx):
    k, n = 7, 128
    rng = np.random.default_rng(55)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=100)) * 6 for _ in range(n)]
    # the queries' hot list: bins with count - 1 >= 2, i.e. k-mers that occur at least twice, over the block of 128 queries
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    hot = 0
    for s in seqs:
        v = np.array([code[c] for c in s], dtype=np.int64)
        kmers = sum(v[i:len(v) - k + 1 + i] << (2 * (k - 1 - i)) for i in range(k))
        _, occ = np.unique(kmers, return_counts=True)
        hot += int((occ >= 2).sum())
    assert hot > 64 * (4 ** k // 128), hot
    sp = api.HistogramSet(ctx, k, 32, n, sparse_entries=sum(len(s) for s in seqs) + 1024)
    sp.build(seqs)
    feat = api.Feature.from_text(ctx, _text(k, 32), 0)
    q_slots = np.arange(n, dtype=np.uint32)
    kw = dict(feat_mask=FAST_MASK, want=WANT)
    on, kernel = _multi(ctx, True, feat, sp, q_slots, q_slots, **kw)
    assert kernel in SPARSE_KERNELS, kernel
    off, k_off = _multi(ctx, False, feat, sp, q_slots, q_slots, **kw)
    assert k_off in SPARSE_KERNELS, k_off          # (either list pass: the set's rank lists are built at the third call that asks for them)
    _same(on, off, "declined block")


def _hot_bins(seq, k):
    """bins of a sequence with count - 1 >= 2: its k-mers that occur at least twice (the length of its list of large bins)"""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    v = np.array([code[c] for c in seq], dtype=np.int64)
    kmers = sum(v[i:len(v) - k + 1 + i] << (2 * (k - 1 - i)) for i in range(k))
    return int((np.unique(kmers, return_counts=True)[1] >= 2).sum())


@pytest.fixture(scope="module")
def declining_case(ctx):
    """140 plain sequences (slots 0 .. 139), then 100 tandem repeats of ~147 large bins each: a block made of the latter has too long a hot list"""
    k, n_plain, n_rep = 7, 140, 100
    rng = np.random.default_rng(57)
    plain, _ = synth.families(5307, n_plain, 600, family=5, length_jitter=40)
    reps = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=150)) * 4 for _ in range(n_rep)]
    seqs = [bytes(s) for s in plain] + reps
    sp, de = _sets(ctx, seqs, k, 32)
    return dict(sp=sp, de=de, feat=api.Feature.from_text(ctx, _text(k, 32), 0), cands=np.arange(len(seqs), dtype=np.uint32), hot=np.array([_hot_bins(s, k) for s in seqs]),
                limit=64 * (4 ** k // 128), rep0=n_plain)


def test_a_block_declines_inside_a_queued_call(ctx, declining_case):
    """blocks of one call that take different routes: plain queries on the matrix cores, tandem-repeat queries whose hot list is too long
    on the list passes (the queued blocks are waited for first), in the middle of the call (a block of 128, cut into two of 64) and at its
    end (a block of 60)"""
    sp, de, feat, cands, hot, limit, rep0 = (declining_case[x] for x in ("sp", "de", "feat", "cands", "hot", "limit", "rep0"))
    middle = np.concatenate([np.arange(128), rep0 + np.arange(100), 100 + np.arange(28), np.arange(12)]).astype(np.uint32)      # 128 | 100 + 28 | 12
    at_end = np.concatenate([np.arange(128), rep0 + 40 + np.arange(60)]).astype(np.uint32)                                      # 128 | 60
    assert hot[middle[:128]].sum() <= limit and hot[middle[128:256]].sum() > limit and hot[middle[256:]].sum() <= limit
    assert hot[at_end[:128]].sum() <= limit and hot[at_end[128:]].sum() > limit
    kw = dict(feat_mask=FAST_MASK, want=WANT)
    for q_slots, last_on_matrix in ((middle, True), (at_end, False)):
        on, kernel = _multi(ctx, True, feat, sp, cands, q_slots, **kw)
        assert kernel.startswith(GEMM) if last_on_matrix else kernel in SPARSE_KERNELS, kernel          # (the name is the last block's)
        off, k_off = _multi(ctx, False, feat, sp, cands, q_slots, **kw)
        assert k_off in SPARSE_KERNELS, k_off
        _same(on, off, ("switch off", last_on_matrix))
        dense, _ = _multi(ctx, True, feat, de, cands, q_slots, **kw)
        _same(on, dense, ("dense", last_on_matrix))


def test_the_second_block_of_192_declines_while_the_first_is_queued(ctx, declining_case):
    """128 plain queries, queued on the matrix cores, then a block of 64 tandem-repeat queries whose hot list is too long: it waits for the
    queued block and runs on the list passes as one block of 64"""
    sp, feat, cands, hot, limit, rep0 = (declining_case[x] for x in ("sp", "feat", "cands", "hot", "limit", "rep0"))
    q_slots = np.concatenate([np.arange(128), rep0 + np.arange(64)]).astype(np.uint32)
    assert q_slots.size == 192 and hot[q_slots[:128]].sum() <= limit and hot[q_slots[128:]].sum() > limit
    kw = dict(feat_mask=FAST_MASK, want=WANT)
    on, kernel = _multi(ctx, True, feat, sp, cands, q_slots, **kw)
    assert kernel in SPARSE_KERNELS, kernel          # (the name is the last block's)
    first, k_first = _multi(ctx, True, feat, sp, cands, q_slots[:130], **kw)          # (the same first block did take the matrix cores: two blocks, 128 | 2)
    assert k_first.startswith(GEMM), k_first
    off, k_off = _multi(ctx, False, feat, sp, cands, q_slots, **kw)
    assert k_off in SPARSE_KERNELS, k_off
    _same(on, off, "192 queries, the second block declined")
    assert np.array_equal(on["counts"], on["close"].sum(axis=1, dtype=np.uint64))


# ------------------------------------------------------------------------------------------------ E. staleness
def test_every_writer_of_a_list_makes_the_mirrors_stale(ctx):
    k, dtype, cap, n = 9, 32, 100, 70          # slots 70 .. 99 never written: 70 .. 95 inside the used block of 32 that starts at 64
    seqs, _ = synth.families(5304, n, 1000, family=5, length_jitter=100)
    seqs = _repeat_bearing(seqs, 7, "unit12")
    other, _ = synth.families(5305, 12, 1000, family=3, length_jitter=100)
    other = _repeat_bearing(other, 3, "di")
    sp = api.HistogramSet(ctx, k, dtype, cap, sparse_entries=4 * sum(len(s) for s in seqs) + 16 * 1400 + 4096)      # the arena is append-only: every rewrite below takes new entries
    sp.build(seqs)
    src = api.HistogramSet(ctx, k, dtype, len(other), sparse_entries=sum(len(s) for s in other) + 1024)
    src.build(other)
    feat = api.Feature.from_text(ctx, _text(k, dtype), 0)
    cands = np.arange(n, dtype=np.uint32)
    q_slots = np.array([1, 3, 10, 11, 20, 33, 40, 41, 42, 64, 65, 69, 0, 8], dtype=np.uint32)
    kw = dict(feat_mask=FAST_MASK, want=WANT)

    def check(where):
        on, kernel = _multi(ctx, True, feat, sp, cands, q_slots, **kw)
        assert kernel.startswith(GEMM), (kernel, where)
        off, k_off = _multi(ctx, False, feat, sp, cands, q_slots, **kw)
        assert k_off in SPARSE_KERNELS, (k_off, where)
        _same(on, off, where)
        return on

    first = check("unwritten slots in a used block")
    sp.build(other[:2], first_slot=10)
    after = check("rebuild of two slots")
    assert not np.array_equal(first["raw"], after["raw"])          # (the rewritten slots are queries and candidates: the results did move)
    sp.assign_from(3, src, 4)
    sp.clone_from(40, src, 7)
    check("assign, clone")
    sp.copy_from(41, src, 1)
    sp.copy_batch([42, 64, 69], src, [2, 5, 10])
    check("copy, copy_batch")
    sp.clear()
    sp.build(seqs[::-1])
    last = check("clear and a full rebuild")
    assert not np.array_equal(after["raw"], last["raw"])


def test_reset_and_unpack_make_the_mirrors_stale(ctx):
    """msc_hist_set_reset forgets every list, msc_hist_unpack (one slot, and batched) writes some again: the slots that stay empty share
    blocks of 32 with the rewritten ones"""
    k, dtype, n = 9, 32, 70
    seqs, _ = synth.families(5309, n, 1000, family=5, length_jitter=100)
    seqs = _repeat_bearing(seqs, 7, "di")
    other, _ = synth.families(5310, 8, 1000, family=4, length_jitter=100)
    other = _repeat_bearing(other, 3, "unit12")
    sp = api.HistogramSet(ctx, k, dtype, n, sparse_entries=sum(len(s) for s in seqs) + 1024)
    sp.build(seqs)
    src = api.HistogramSet(ctx, k, dtype, len(other), sparse_entries=sum(len(s) for s in other) + 1024)
    src.build(other)
    feat = api.Feature.from_text(ctx, _text(k, dtype), 0)
    kw = dict(feat_mask=FAST_MASK, want=WANT)
    everyone = np.arange(n, dtype=np.uint32)
    on, kernel = _multi(ctx, True, feat, sp, everyone, everyone[:9], **kw)          # the mirrors stand
    assert kernel.startswith(GEMM), kernel
    offs, at = [], 0
    for s_ in range(len(other)):
        offs.append(at)
        at += src.packed_bytes(s_)
    dev = ctx.device_malloc(at)
    try:
        src.pack(np.arange(len(other)), dev, offs)
        sp.reset()
        dst = [2, 5, 6, 40, 41, 69, 33, 0]
        sp.unpack([dst[0]], dev, [offs[0]])
        sp.unpack(dst[1:], dev, offs[1:])
    finally:
        ctx.synchronize()
        ctx.device_free(dev)
    slots = np.array(dst, dtype=np.uint32)
    q_slots = np.array([2, 40, 69, 0, 5, 5], dtype=np.uint32)
    on, kernel = _multi(ctx, True, feat, sp, slots, q_slots, **kw)
    assert kernel.startswith(GEMM), kernel
    off, k_off = _multi(ctx, False, feat, sp, slots, q_slots, **kw)
    assert k_off in SPARSE_KERNELS, k_off
    _same(on, off, "reset, unpack")
    back = {d: i for i, d in enumerate(dst)}          # the same pairs in the set the slots came from
    ref, _ = _multi(ctx, False, feat, src, np.arange(len(other), dtype=np.uint32), np.array([back[int(q)] for q in q_slots], dtype=np.uint32), **kw)
    _same(on, ref, "the source set")


# ------------------------------------------------------------------------------------------------ F. search_pairs
@pytest.fixture(scope="module")
def pairs_case(ctx):
    seqs, _ = synth.families(5306, 180, 1000, family=10, length_jitter=120)
    runs = [b"A" * 300, b"AC" * 150, b"ACGTTGCAAGTC" * 10]
    seqs = [bytes(s[:200 + i]) + runs[(i // 9) % 3] + bytes(s[200 + i:]) if i % 9 == 4 else bytes(s) for i, s in enumerate(seqs)]
    sp, de = _sets(ctx, seqs, 9, 32)
    return dict(sp=sp, de=de, n=len(seqs), q=np.arange(140, dtype=np.uint32))          # blocks of 128 + 12


def _pairs(ctx, pred, on, cells, hs, q, n, **kw):
    ctx.set_sparse_matrix_pass(on)
    ctx.set_pairs_div_cells(cells)
    try:
        got = pred.search_pairs(hs, None, hs, q, m=n, **kw)
        return got, ctx.last_kernel_info()[0]
    finally:
        ctx.set_sparse_matrix_pass(False)
        ctx.set_pairs_div_cells(False)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("windows", [False, True], ids=["whole", "windows"])
def test_search_pairs_takes_the_matrix_route(ctx, pairs_case, windows):
    sp, de, n, q = pairs_case["sp"], pairs_case["de"], pairs_case["n"], pairs_case["q"]
    pred = api.Predictor.from_text(ctx, weights_text("weights_k9_u32_fc.txt"))
    kw = {}
    if windows:
        rng = np.random.default_rng(56)
        lo = rng.integers(0, n, size=q.size).astype(np.uint64)
        hi = np.minimum(lo + rng.integers(1, 120, size=q.size), n + 5).astype(np.uint64)
        lo[::17] = hi[::17]          # some empty
        kw = dict(win_lo=lo, win_hi=hi)
    on, kernel = _pairs(ctx, pred, True, False, sp, q, n, **kw)
    assert on[3]["route"] == api.PAIRS_ROUTE_MATRIX, on[3]
    assert kernel.startswith(GEMM) and "mirrors from lists" in kernel, kernel
    off, _ = _pairs(ctx, pred, False, False, sp, q, n, **kw)
    assert off[3]["route"] == api.PAIRS_ROUTE_FALLBACK, off[3]
    dense, _ = _pairs(ctx, pred, False, False, de, q, n, **kw)
    assert dense[3]["route"] == api.PAIRS_ROUTE_MATRIX, dense[3]
    assert on[3]["n_pairs"] > (0 if windows else q.size // 2)
    for other, where in ((off, "switch off"), (dense, "dense")):
        assert np.array_equal(on[0], other[0]) and np.array_equal(on[1], other[1]), where
        assert np.array_equal(_bits(on[2]), _bits(other[2])), where


# ------------------------------------------------------------------------------------------------ G. the cells form
def _two_block(text):
    """the class block of a `mode: 1` file twice, as a `mode: 3` file: the regression block is the same slow model"""
    head, block = text.split("\nn_combos:", 1)
    block = "\nn_combos:" + block.rstrip("\n") + "\n"
    return head.replace("mode: 1", "mode: 3") + block + block


def test_cells_form_on_sparse_sets(ctx, pairs_case):
    sp, de, n, q = pairs_case["sp"], pairs_case["de"], pairs_case["n"], pairs_case["q"]
    text = _two_block(weights_text("weights_cfg5_k9.txt").replace("uint8_t", "uint32_t"))
    pred = api.Predictor.from_text(ctx, text)
    on, kernel = _pairs(ctx, pred, True, True, sp, q, n)
    assert on[3]["route"] == api.PAIRS_ROUTE_MATRIX, on[3]
    assert kernel.startswith(GEMM) and "divergence sums from cells" in kernel and "mirrors from lists" in kernel, kernel
    dense, _ = _pairs(ctx, pred, False, True, de, q, n)
    assert dense[3]["route"] == api.PAIRS_ROUTE_MATRIX
    assert np.array_equal(on[0], dense[0]) and np.array_equal(on[1], dense[1]) and np.array_equal(_bits(on[2]), _bits(dense[2]))      # same mirrors, same order of additions
    # next to the switch-off call (the merge kernels' sums): the pairs both list agree to 1e-9; a pair only one lists sits within 1e-9 of the threshold
    off, _ = _pairs(ctx, pred, False, False, sp, q, n)
    assert off[3]["route"] == api.PAIRS_ROUTE_FALLBACK
    sums = api.score_multi(ctx, pred.cls, sp, None, sp, q, m=n, want=("sum",))["sum"]          # the classifier's weighted sums, today's route: close iff sum >= 0
    key = lambda r: np.repeat(np.arange(q.size, dtype=np.int64), np.diff(r[0].astype(np.int64))) * n + r[1].astype(np.int64)
    k_on, k_off = key(on), key(off)
    both, i_on, i_off = np.intersect1d(k_on, k_off, assume_unique=True, return_indices=True)
    assert both.size > q.size // 2
    assert np.all(np.abs(on[2][i_on] - off[2][i_off]) <= RTOL * np.abs(off[2][i_off]))
    for only in np.setxor1d(k_on, k_off, assume_unique=True):
        assert abs(sums[only // n, only % n]) <= 1e-9, (int(only // n), int(only % n), sums[only // n, only % n])


# ------------------------------------------------------------------------------------------------ H. guards
@pytest.mark.parametrize("why", ["dtype64", "one_query", "jensen_shannon"])
def test_guards_keep_todays_route(ctx, why):
    seqs, _ = synth.families(5308, 40, 1000, family=5, length_jitter=100)
    seqs = [bytes(s) for s in seqs]
    dtype = 64 if why == "dtype64" else 32
    sp = api.HistogramSet(ctx, 9, dtype, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 1024)
    sp.build(seqs)
    if why == "jensen_shannon":
        feat = api.Feature.from_text(ctx, weights_text("weights_cfg5_k9.txt").replace("uint8_t", "uint32_t"), 0)
        js = dict(FEATS)["jensen_shannon"]
        assert any(f & (1 << js) for f in feat.single_flags())
    else:
        feat = api.Feature.from_text(ctx, _text(9, dtype), 0)
    q_slots = np.arange(1 if why == "one_query" else 12, dtype=np.uint32)
    cands = np.arange(len(seqs), dtype=np.uint32)
    kw = dict(feat_mask=FAST_MASK, want=("sum", "csum", "close"))
    on, kernel = _multi(ctx, True, feat, sp, cands, q_slots, **kw)
    off, k_off = _multi(ctx, False, feat, sp, cands, q_slots, **kw)
    assert not kernel.startswith(GEMM) and not k_off.startswith(GEMM), (kernel, k_off)
    if why == "dtype64":          # (several list kernels are possible here: the set's rank lists are built at the third call that asks for them)
        assert kernel in SPARSE_KERNELS and k_off in SPARSE_KERNELS, (kernel, k_off)
    _same(on, off, why, keys=("raw", "sum", "csum", "close"))


# ------------------------------------------------------------------------------------------------ I. msc_fastcar
def test_fastcar_sparse_matrix_reproduces_the_reference_output(tmp_path):
    """the inputs of test_fastcar_k9_u32_reproduces_reference_output_on_the_matrix_cores (tests/test_gpu_qxm_direct.py), sparse sets"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "meshclust2_amd", "host", "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "meshclust2_amd", "host")])
    db, h = synth.families(43, 220, 1000, family=10, length_jitter=120)
    q, hq = synth.families(43, 30, 1000, family=10, length_jitter=120)
    runs = [b"A" * 300, b"AC" * 150, b"ACGTTGCAAGTC" * 10]
    db = [s[:200 + i] + runs[(i // 9) % 3] + s[200 + i:] if i % 9 == 4 else s for i, s in enumerate(db)]
    q = [x[:len(x) - 5] for x in q]
    q[4] = q[4][:333] + runs[0] + q[4][333:]
    synth.write_fasta(str(tmp_path / "db.fa"), db, h)
    synth.write_fasta(str(tmp_path / "q.fa"), q, [x.replace(">seq", ">qry") for x in hq])
    golden = os.path.join(root, "tests", "golden")
    r = subprocess.run([exe, "db.fa", "--query", "q.fa", "--recover", os.path.join(golden, "weights_k9_u32_fc.txt"), "--output", "fc_out", "--sparse", "--sparse-matrix", "--kernels"],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-2000:]
    got = open(str(tmp_path / "fc_out0"), "rb").read()
    exp = open(os.path.join(golden, "fastcar_k9_u32.out"), "rb").read()
    assert got == exp, "fastcar output differs (%d vs %d bytes)" % (len(got), len(exp))
    kernels = [ln.split(": ", 1)[1] for ln in r.stderr.decode().splitlines() if ln.startswith("kernel: ")]
    assert kernels and all(kn.startswith(GEMM) for kn in kernels), kernels
