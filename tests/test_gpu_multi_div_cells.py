"""msc_set_multi_div_cells: msc_score_multi keeps a block whose model or feat_mask holds jefferey_divergence / jensen_shannon on the
matrix-core route, the two sums evaluated in the epilogue from (count, count) cells and the lists of large bins (bits_pair_div in
pair_features.hip) -- no merge pass per query. Held to the switch-off call (the sparse merge kernels' sums): integer statistics bit for bit,
the two sums and what a model derives from them to rounding; to the CPU oracle; and to itself and to msc_search_pairs under
msc_set_pairs_div_cells bit for bit whatever the slot list, the number of queries, the block pipe, the chunks of candidates or the layout of
the sets. Default off: the parent's kernels and bits.

The input is a smaller version of tests/test_gpu_search_pairs_div.py's: 300 sequences of 192 .. 702 bases, 140 queries (blocks of 128 + 12)
x 300 candidates (two whole 128-candidate tiles and a short one). It has no pair near the threshold (asserted below on the switch-off
call's own sums), so no flag may differ between the routes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import FEAT_BIT, weights_text, weights_with_mode
from meshclust2_amd import api, synth
from test_gpu_search_pairs_div import GROUPS_TEXT, _set, _spliced, _two_block, _unclamped

pytestmark = pytest.mark.gpu
GEMM = "k_pair_gemm_fp4_dma<"
CELLS = "divergence sums from cells"
RTOL, ATOL = 1e-9, 1e-13          # the tolerances of tests/test_gpu_qxm_direct.py and tests/test_gpu_search_pairs_div.py
NQ, N = 140, 300
COLS = ["manhattan", "jefferey_divergence", "emd", "jensen_shannon"]          # ascending bit order: the columns of raw_out
MASK = sum(1 << FEAT_BIT[name] for name in COLS)
INT_COLS, DIV_COLS = [0, 2], [1, 3]
ORDERS = (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST)
WANT = ("sum", "csum", "close", "counts")


def _sequences():
    seqs, _ = synth.families(6160, N, 300, family=20, length_jitter=120)
    return _spliced(seqs)


def _close_enough(got, exp):
    return np.abs(got - exp) <= ATOL + RTOL * np.abs(exp)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _multi(ctx, on, *args, **kw):
    """score_multi with the switch set for this call -> (result, kernel name)"""
    ctx.set_multi_div_cells(on)
    try:
        got = api.score_multi(ctx, *args, **kw)
    finally:
        ctx.set_multi_div_cells(False)
    return got, ctx.last_kernel_info()[0]


def _sample():
    """every pair of two spliced queries, and a pair inside every family (the first seven) or across to it (the others: their members are
    candidates only) -> [(query, candidate)]"""
    spliced = [i for i in range(NQ) if i % 9 == 4]
    pairs = [(a, b) for a in spliced for b in spliced if a < b]
    pairs += [(20 * f, 20 * f + 1) if 20 * f < NQ else ((7 * f + 3) % NQ, 20 * f + 1) for f in range(N // 20)]
    assert 130 <= len(pairs) <= 160
    return pairs


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seqs():
    return _sequences()


@pytest.fixture(scope="module")
def lin_text():
    return weights_with_mode(_unclamped(_two_block(weights_text("weights_cfg5_k9.txt"))), 2)


@pytest.fixture(scope="module", params=[8, 16], ids=["u8", "u16"])
def case(request, ctx, seqs, lin_text):
    """a set, the slow model, and per argument order the switch-off and switch-on calls: computed once, left unchanged"""
    hs = _set(ctx, seqs, 9, request.param)
    q = np.arange(NQ, dtype=np.uint32)
    feat = api.Feature.from_text(ctx, weights_text("weights_cfg5_k9.txt"), 0)
    lin = api.Predictor.from_text(ctx, lin_text)
    off, on, on_status, on_counts = {}, {}, {}, {}
    for order in ORDERS:
        off[order] = _multi(ctx, False, feat, hs, None, hs, q, order=order, m=N, feat_mask=MASK, want=WANT)
        on[order] = _multi(ctx, True, feat, hs, None, hs, q, order=order, m=N, feat_mask=MASK, want=WANT)
        counts = np.zeros(NQ, dtype=np.uint64)          # the device's own counts of the switch-on call, and whether it kept them
        on_status[order] = ctx.lib.msc_last_close_counts(ctx.h, api._ptr(counts), NQ)
        on_counts[order] = counts
    # the margin of this input, on the switch-off call's own sums: no pair sits where rounding could move its flag, and both flags occur
    for order in ORDERS:
        s = off[order][0]["sum"]
        assert s.shape == (NQ, N) and np.min(np.abs(s)) > 1e-6, np.min(np.abs(s))
        assert 1000 < int(off[order][0]["close"].sum()) < NQ * N - 1000
    # the unclamped regression-only model with the switch on: the sums the bit comparisons are held to
    plain, name = _multi(ctx, True, lin.reg, hs, None, hs, q, m=N, want=("sum",))
    assert name.startswith(GEMM) and CELLS in name, name
    return dict(dtype=request.param, hs=hs, q=q, feat=feat, lin=lin, off=off, on=on, on_status=on_status, on_counts=on_counts, plain=plain["sum"].copy())


@pytest.mark.parametrize("order", ORDERS, ids=["cand_first", "query_first"])
def test_switch_on_stays_on_the_matrix_route_and_agrees_with_switch_off(case, order):
    (off, off_name), (on, on_name) = case["off"][order], case["on"][order]
    assert on_name.startswith(GEMM) and CELLS in on_name, on_name
    assert CELLS not in off_name, off_name
    assert np.array_equal(on["close"], off["close"])
    assert case["on_status"][order] == 0          # msc_last_close_counts answers for the call
    assert np.array_equal(case["on_counts"][order], on["close"].sum(axis=1, dtype=np.uint64))
    assert np.array_equal(on["counts"], case["on_counts"][order])
    for key in ("sum", "csum"):
        ok = _close_enough(on[key], off[key])
        assert ok.all(), (key, int((~ok).sum()), float(np.max(np.abs(on[key] - off[key]))))
    assert on["raw"].shape == (NQ, N, len(COLS))
    for col in INT_COLS:
        assert np.array_equal(on["raw"][..., col], off["raw"][..., col]), COLS[col]
    for col in DIV_COLS:
        ok = _close_enough(on["raw"][..., col], off["raw"][..., col])
        assert ok.all(), (COLS[col], int((~ok).sum()))


@pytest.mark.parametrize("order", ORDERS, ids=["cand_first", "query_first"])
def test_a_fixed_sample_against_the_oracle(case, seqs, oracle, order):
    on = case["on"][order][0]
    sample = _sample()
    model = oracle.predictor(weights_text("weights_cfg5_k9.txt")).cls
    hist = {i: oracle.hist(seqs[i], 9, case["dtype"]) for i in sorted({i for p in sample for i in p})}
    for qi, ci in sample:
        a, b = (hist[ci], hist[qi]) if order == api.ORDER_CAND_FIRST else (hist[qi], hist[ci])
        for col, name in enumerate(COLS):
            want = oracle.raw_feature(1 << FEAT_BIT[name], a, b)
            got = on["raw"][qi, ci, col]
            if col in INT_COLS:
                assert got == want, (name, qi, ci)
            else:
                assert abs(got - want) <= ATOL + RTOL * abs(want), (name, qi, ci, got, want)
        want = oracle.score(model, a, b)[2]
        assert abs(on["sum"][qi, ci] - want) <= ATOL + RTOL * abs(want), (qi, ci, on["sum"][qi, ci], want)
        assert on["close"][qi, ci] == (1 if want >= 0 else 0), (qi, ci, want)
    for h in hist.values():
        oracle.lib().orc_hist_free(h)


def test_a_pairs_bits_do_not_depend_on_the_call(ctx, case, seqs):
    hs, q, reg, plain = case["hs"], case["q"], case["lin"].reg, case["plain"]
    # a permuted slot list, and one with repeats
    rng = np.random.default_rng(11)
    for slots in (rng.permutation(N).astype(np.uint32), rng.integers(0, N, size=350).astype(np.uint32)):
        got, name = _multi(ctx, True, reg, hs, slots, hs, q, want=("sum",))
        assert name.startswith(GEMM) and CELLS in name, name
        assert np.array_equal(_bits(got["sum"]), _bits(plain[:, slots]))
    # 130 queries: blocks of 128 + 2 instead of 128 + 12
    got, name = _multi(ctx, True, reg, hs, None, hs, q[:130], m=N, want=("sum",))
    assert name.startswith(GEMM) and CELLS in name, name
    assert np.array_equal(_bits(got["sum"]), _bits(plain[:130]))
    # every kernel of a block on one stream
    ctx.set_block_pipe(False)
    try:
        got, name = _multi(ctx, True, reg, hs, None, hs, q, m=N, want=("sum",))
    finally:
        ctx.set_block_pipe(True)
    assert name.startswith(GEMM) and CELLS in name, name
    assert np.array_equal(_bits(got["sum"]), _bits(plain))
    # msc_search_pairs under its own switch (this one off): every pair listed, its similarity the unclamped sum
    ctx.set_pairs_div_cells(True)
    try:
        listed = case["lin"].search_pairs(hs, None, hs, q, m=N)
    finally:
        ctx.set_pairs_div_cells(False)
    assert listed[3]["route"] == api.PAIRS_ROUTE_MATRIX and listed[3]["n_pairs"] == NQ * N
    assert np.all((plain > 0) & (plain < 1))          # (nothing clamped)
    assert np.array_equal(_bits(listed[2].reshape(NQ, N)), _bits(plain))
    # the same sequences in two sparse sets on the matrix-core route
    sp = _set(ctx, seqs, 9, case["dtype"], sparse=True)
    ctx.set_sparse_matrix_pass(True)
    try:
        got, name = _multi(ctx, True, reg, sp, None, sp, q, m=N, want=("sum",))
    finally:
        ctx.set_sparse_matrix_pass(False)
    assert name.startswith(GEMM) and CELLS in name and "mirrors from lists" in name, name
    assert np.array_equal(_bits(got["sum"]), _bits(plain))


_CHUNKED = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
from meshclust2_amd import api, synth
from golden_util import weights_text, weights_with_mode
from test_gpu_search_pairs_div import _spliced, _two_block, _unclamped
ctx = api.Context(0)
seqs, _ = synth.families(6161, 300, 200, family=20, length_jitter=30)
seqs = _spliced(seqs)
hs = api.HistogramSet(ctx, 9, 8, len(seqs))
for off in range(0, len(seqs), 256):
    hs.build(seqs[off:off + 256], first_slot=off)
reg = api.Predictor.from_text(ctx, weights_with_mode(_unclamped(_two_block(weights_text("weights_cfg5_k9.txt"))), 2)).reg
ctx.set_multi_div_cells(True)
q = np.arange(130, dtype=np.uint32)
plain = api.score_multi(ctx, reg, hs, None, hs, q, m=len(seqs), want=("sum",))["sum"]
name = ctx.last_kernel_info()[0]
assert name.startswith("k_pair_gemm_fp4_dma<") and "divergence sums from cells" in name, name
# 70 000 candidates (slots of the set, repeated): with 64 slices and 128 query rows the product array holds 65 536, so two chunks of 35 000 run
slots = np.random.default_rng(5).integers(0, len(seqs), size=70000).astype(np.uint32)
got = api.score_multi(ctx, reg, hs, slots, hs, q, want=("sum",))["sum"]
name = ctx.last_kernel_info()[0]
assert name.startswith("k_pair_gemm_fp4_dma<") and "divergence sums from cells" in name, name
assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(plain[:, slots]).view(np.uint64))
print("ok", got.size)
"""


def test_candidates_in_several_chunks_give_the_same_bits():
    """MSC_GEMM_SLICES is read once per process: a child process, as tests/test_gpu_search_pairs_div.py does"""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MSC_GEMM_SLICES="64")
    r = subprocess.run([sys.executable, "-c", _CHUNKED, os.path.dirname(tests), tests], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"ok" in r.stdout, r.stdout.decode(errors="replace")[-3000:]


def test_a_dense_set_on_the_route_builds_no_sparse_mirror(ctx, seqs):
    hs = _set(ctx, seqs, 9, 8)          # fresh: no call has touched it
    feat = api.Feature.from_text(ctx, weights_text("weights_cfg5_k9.txt"), 0)
    q = np.arange(NQ, dtype=np.uint32)
    _, name = _multi(ctx, True, feat, hs, None, hs, q, m=N, want=("close",))
    assert name.startswith(GEMM) and CELLS in name, name
    assert hs.entries(0) == 0          # (a dense set reports its sparse mirror's stored bins: 0 before the mirror exists)
    _, name = _multi(ctx, False, feat, hs, None, hs, q, m=N, want=("close",))
    assert hs.entries(0) > 0, name     # the switch-off call's merge passes read the mirror


def test_a_block_that_falls_back_has_the_merge_kernels_bits_and_the_others_the_cells(ctx, seqs):
    """Queries 128 .. 255 are a 1 300-base unit three times over: about 1 300 large bins each, 166 000 in their block's hot list where
    the bound at k = 9 is 64 x 2 048 = 131 072, so that block leaves the matrix cores -- after block 0 was queued on them and before block
    2 is. It is then scored as with the switch off (the sparse mirrors are built for it, not before), the two other blocks from cells."""
    rng = np.random.default_rng(77)
    heavy = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 1300)) * 3 for _ in range(128)]
    hs = _set(ctx, seqs[:128] + heavy + seqs[128:140], 9, 8)
    feat = api.Feature.from_text(ctx, weights_text("weights_cfg5_k9.txt"), 0)
    cands = np.concatenate([np.arange(100), np.arange(128, 178)]).astype(np.uint32)          # plain and heavy candidates
    q_all = np.arange(268, dtype=np.uint32)
    plain_rows = np.concatenate([np.arange(128), np.arange(256, 268)])
    # the plain queries alone: blocks of 128 + 12, both from cells, no mirror
    on_plain, name = _multi(ctx, True, feat, hs, cands, hs, q_all[plain_rows], feat_mask=MASK, want=WANT)
    assert name.startswith(GEMM) and CELLS in name, name
    assert hs.entries(0) == 0 and hs.entries(130) == 0
    # all of them: matrix, fall-back (two sub-blocks of 64), matrix
    on, name = _multi(ctx, True, feat, hs, cands, hs, q_all, feat_mask=MASK, want=WANT)
    assert name.startswith(GEMM) and CELLS in name, name          # (the call's last block)
    status = ctx.lib.msc_last_close_counts(ctx.h, api._ptr(np.zeros(268, dtype=np.uint64)), 268)
    assert hs.entries(0) > 0 and hs.entries(130) > 0          # the block that fell back had the mirrors built
    off, off_name = _multi(ctx, False, feat, hs, cands, hs, q_all, feat_mask=MASK, want=WANT)
    assert CELLS not in off_name, off_name
    for key in ("sum", "csum", "raw"):
        assert np.array_equal(_bits(on[key][128:256]), _bits(off[key][128:256])), key          # the merge kernels' bits
        assert np.array_equal(_bits(on[key][plain_rows]), _bits(on_plain[key])), key            # the cells' bits
        ok = _close_enough(on[key], off[key])
        assert ok.all(), (key, int((~ok).sum()))
    assert not np.array_equal(_bits(on["raw"][plain_rows][..., DIV_COLS]), _bits(off["raw"][plain_rows][..., DIV_COLS]))          # (another order of additions)
    for col in INT_COLS:
        assert np.array_equal(on["raw"][..., col], off["raw"][..., col]), COLS[col]
    assert np.min(np.abs(off["sum"])) > 1e-6, np.min(np.abs(off["sum"]))          # no pair where rounding could move its flag
    assert np.array_equal(on["close"], off["close"])
    assert status == 0 and np.array_equal(on["counts"], on["close"].sum(axis=1, dtype=np.uint64))


def test_small_histograms_take_the_route(ctx, seqs, oracle):
    """k = 7 with 16-bit bins: 32 KiB histograms, whole 4 KiB tiles, no list form -- switch off scores them one query at a time"""
    hs = _set(ctx, seqs, 7, 16)
    q = np.arange(NQ, dtype=np.uint32)
    for order in ORDERS:
        off, off_name = _multi(ctx, False, None, hs, None, hs, q, order=order, m=N, feat_mask=MASK)
        on, on_name = _multi(ctx, True, None, hs, None, hs, q, order=order, m=N, feat_mask=MASK)
        assert on_name.startswith(GEMM) and CELLS in on_name, on_name
        assert CELLS not in off_name, off_name
        for col in INT_COLS:
            assert np.array_equal(on["raw"][..., col], off["raw"][..., col]), COLS[col]
        for col in DIV_COLS:
            ok = _close_enough(on["raw"][..., col], off["raw"][..., col])
            assert ok.all(), (COLS[col], int((~ok).sum()))
        sample = _sample()
        hist = {i: oracle.hist(seqs[i], 7, 16) for i in sorted({i for p in sample for i in p})}
        for qi, ci in sample:
            a, b = (hist[ci], hist[qi]) if order == api.ORDER_CAND_FIRST else (hist[qi], hist[ci])
            for col, name in enumerate(COLS):
                want = oracle.raw_feature(1 << FEAT_BIT[name], a, b)
                got = on["raw"][qi, ci, col]
                if col in INT_COLS:
                    assert got == want, (name, qi, ci)
                else:
                    assert abs(got - want) <= ATOL + RTOL * abs(want), (name, qi, ci, got, want)
        for h in hist.values():
            oracle.lib().orc_hist_free(h)
    assert hs.entries(0) == 0          # (no list form)


@pytest.mark.parametrize("why", ["groups_model", "k5_set", "k13_sparse", "one_query"])
def test_declines_keep_the_switch_off_kernels_and_bits(ctx, why):
    s, _ = synth.families(5150, 60, 1000, family=20)
    if why == "groups_model":
        hs, text = _set(ctx, s, 9, 8), GROUPS_TEXT
    elif why == "k5_set":
        hs, text = _set(ctx, s, 5, 16), weights_text("weights_k5_u16_slow.txt")
    elif why == "k13_sparse":
        hs, text = _set(ctx, s, 13, 64, sparse=True), weights_text("weights_cfg4_k13.txt")
    else:
        hs, text = _set(ctx, s, 9, 8), weights_text("weights_cfg5_k9.txt")
    feat = api.Feature.from_text(ctx, text, 0)
    q = np.arange(1 if why == "one_query" else 40, dtype=np.uint32)
    off, off_name = _multi(ctx, False, feat, hs, None, hs, q, m=len(s), feat_mask=MASK, want=WANT)
    on, on_name = _multi(ctx, True, feat, hs, None, hs, q, m=len(s), feat_mask=MASK, want=WANT)
    assert on_name == off_name and CELLS not in on_name, (on_name, off_name)
    for key in ("sum", "csum", "raw"):
        assert np.array_equal(_bits(on[key]), _bits(off[key])), key
    assert np.array_equal(on["close"], off["close"]) and np.array_equal(on["counts"], off["counts"])


def test_on_then_off_gives_the_parents_bits(ctx, case):
    hs, q, feat = case["hs"], case["q"], case["feat"]
    off, off_name = case["off"][api.ORDER_CAND_FIRST]
    on, on_name = _multi(ctx, True, feat, hs, None, hs, q, m=N, feat_mask=MASK, want=WANT)
    assert CELLS in on_name
    again, name = _multi(ctx, False, feat, hs, None, hs, q, m=N, feat_mask=MASK, want=WANT)
    assert name == off_name, (name, off_name)
    for key in ("sum", "csum", "raw"):
        assert np.array_equal(_bits(again[key]), _bits(off[key])), key
    assert np.array_equal(again["close"], off["close"]) and np.array_equal(again["counts"], off["counts"])
