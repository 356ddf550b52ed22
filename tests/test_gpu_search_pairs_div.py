"""msc_set_pairs_div_cells: msc_search_pairs keeps a model that holds jefferey_divergence / jensen_shannon (every --feat slow model) on the
matrix-core route, the two sums evaluated per pair from (count, count) cells and the lists of large bins (bits_pair_div in pair_features.hip).
Held to the fallback route (the sparse merge kernels' sums): the same pairs, similarities to rounding; to the CPU oracle; and to itself bit for
bit whatever the slot list, the windows, the number of queries or the chunks of candidates. Default off: the parent's list, bit for bit.

The input has no pair near the threshold (asserted below on the fallback route's own sums), so no flag may differ between the routes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import weights_text, weights_with_mode
from meshclust2_amd import api, synth

pytestmark = pytest.mark.gpu
GEMM = "k_pair_gemm_fp4_dma<"
RTOL, ATOL = 1e-9, 1e-13          # the tolerances of tests/test_gpu_qxm_direct.py
RUNS = [b"A" * 300, b"AC" * 150, b"ACGTTGCAAGTC" * 10]          # the repeat runs of test_reference_fastcar_bytes_from_the_new_call
NQ = 140          # blocks of 128 + 12

GROUPS_TEXT = """k: 9
mode: 1
max_features: 4
ID: 0.6
Datatype: uint8_t
feature_set: 65664

n_combos: 2
-0.4
0 65536 1.7
0 128 -0.9

n_singles: 2
128 0 0.5
65536 0 0.02
"""


def _spliced(seqs):
    """large bins on both sides, shared large bins, a bin past 255, unequal magnitudes"""
    return [s[:200 + i] + RUNS[(i // 9) % 3] + s[200 + i:] if i % 9 == 4 else s for i, s in enumerate(seqs)]


def _sequences():
    seqs, _ = synth.families(6160, 300, 1000, family=20, length_jitter=120)
    return _spliced(seqs)


def _two_block(text):
    """the class block of a `mode: 1` file twice, as a `mode: 3` file: the regression block is the same slow model"""
    head, block = text.split("\nn_combos:", 1)
    block = "\nn_combos:" + block.rstrip("\n") + "\n"
    return head.replace("mode: 1", "mode: 3") + block + block


def _unclamped(text):
    """the two-block text with the regression block's weights scaled by 1 / 4 and its sum moved by 0.4: the same statistics and combinations,
    and every sum of this input (-0.8 .. 1.6 before) strictly inside [0, 1], where p_predict's clamp hides nothing"""
    head, cls_block, reg_block = text.split("\nn_combos:")
    lines = reg_block.split("\n")
    n = int(lines[0])
    lines[1] = repr(0.4 + 0.25 * float(lines[1]))
    for i in range(2, 2 + n):
        kind, flags, w = lines[i].split()
        lines[i] = "%s %s %r" % (kind, flags, 0.25 * float(w))
    return "\nn_combos:".join([head, cls_block, "\n".join(lines)])


def _set(ctx, seqs, k, dtype, sparse=False):
    hs = api.HistogramSet(ctx, k, dtype, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 1024 if sparse else 0)
    for off in range(0, len(seqs), 256):
        hs.build(seqs[off:off + 256], first_slot=off)
    return hs


def _close_enough(got, exp):
    return np.abs(got - exp) <= ATOL + RTOL * np.abs(exp)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seqs():
    return _sequences()


@pytest.fixture(scope="module")
def text3():
    return _two_block(weights_text("weights_cfg5_k9.txt"))


@pytest.fixture(scope="module", params=[8, 16], ids=["u8", "u16"])
def case(request, ctx, seqs, text3):
    """a set, the two-block and the regression-only predictors, and the switch-off (fallback) lists: computed once, left unchanged"""
    hs = _set(ctx, seqs, 9, request.param)
    n = len(seqs)
    q = np.arange(NQ, dtype=np.uint32)
    pred = api.Predictor.from_text(ctx, text3)
    pred_reg = api.Predictor.from_text(ctx, weights_with_mode(text3, 2))
    pred_lin = api.Predictor.from_text(ctx, weights_with_mode(_unclamped(text3), 2))
    ctx.set_pairs_div_cells(False)
    off = pred.search_pairs(hs, None, hs, q, m=n)
    off_reg = pred_reg.search_pairs(hs, None, hs, q, m=n)
    off_lin = pred_lin.search_pairs(hs, None, hs, q, m=n)
    assert off[3]["route"] == off_reg[3]["route"] == off_lin[3]["route"] == api.PAIRS_ROUTE_FALLBACK
    # the margin of this input, on the fallback route's own sums: no pair sits where rounding could move its flag
    s = api.score_multi(ctx, pred.cls, hs, None, hs, q, m=n, want=("sum",))["sum"]
    assert s.shape == (NQ, n) and np.min(np.abs(s)) > 1e-6, np.min(np.abs(s))
    assert 1000 < off[3]["n_pairs"] < NQ * n and off_reg[3]["n_pairs"] == off_lin[3]["n_pairs"] == NQ * n
    assert np.all((off_lin[2] > 0) & (off_lin[2] < 1))          # (nothing clamped)
    return dict(dtype=request.param, hs=hs, n=n, q=q, pred=pred, pred_reg=pred_reg, pred_lin=pred_lin, off=off, off_reg=off_reg, off_lin=off_lin)


@pytest.fixture(scope="module")
def plain(ctx, case):
    """the regression-only model (unclamped form) with the switch on: every pair listed, sim [NQ][n]"""
    ctx.set_pairs_div_cells(True)
    try:
        got = case["pred_lin"].search_pairs(case["hs"], None, case["hs"], case["q"], m=case["n"])
    finally:
        ctx.set_pairs_div_cells(False)
    assert got[3]["route"] == api.PAIRS_ROUTE_MATRIX and got[3]["n_pairs"] == NQ * case["n"]
    return got[2].reshape(NQ, case["n"]).copy()


def _on(ctx, pred, *args, **kw):
    ctx.set_pairs_div_cells(True)
    try:
        return pred.search_pairs(*args, **kw)
    finally:
        ctx.set_pairs_div_cells(False)


def test_switch_on_takes_the_matrix_route_and_lists_the_same_pairs(ctx, case):
    hs, n, q = case["hs"], case["n"], case["q"]
    got = _on(ctx, case["pred"], hs, None, hs, q, m=n)
    name = ctx.last_kernel_info()[0]
    assert got[3]["route"] == api.PAIRS_ROUTE_MATRIX, got[3]
    assert name.startswith(GEMM) and "divergence sums from cells" in name, name
    off = case["off"]
    assert np.array_equal(got[0], off[0]) and np.array_equal(got[1], off[1])
    assert got[3]["n_pairs"] == off[3]["n_pairs"]
    assert got[3]["fp64_pairs"] == NQ * n + got[3]["n_pairs"]          # every pair's flag, every listed pair's similarity
    # the similarities of the listed pairs agree to rounding
    ok = _close_enough(got[2], off[2])
    assert ok.all(), (int((~ok).sum()), float(np.max(np.abs(got[2] - off[2]))))
    # a classification block alone: similarity 1
    cls_only = _on(ctx, api.Predictor.from_text(ctx, weights_text("weights_cfg5_k9.txt")), hs, None, hs, q, m=n)
    assert cls_only[3]["route"] == api.PAIRS_ROUTE_MATRIX and cls_only[3]["fp64_pairs"] == NQ * n
    assert np.array_equal(cls_only[0], off[0]) and np.array_equal(cls_only[1], off[1]) and np.all(cls_only[2] == 1.0)


def test_values_agree_with_the_fallback_and_the_oracle(ctx, case, plain, seqs, oracle, text3):
    hs, n, q = case["hs"], case["n"], case["q"]
    # the slow model itself as the regression block (its sums leave [0, 1] for most pairs: clamped), and its unclamped form
    clamped = _on(ctx, case["pred_reg"], hs, None, hs, q, m=n)
    assert clamped[3]["route"] == api.PAIRS_ROUTE_MATRIX and clamped[3]["n_pairs"] == NQ * n
    clamped = clamped[2].reshape(NQ, n)
    for got, exp in ((clamped, case["off_reg"][2].reshape(NQ, n)), (plain, case["off_lin"][2].reshape(NQ, n))):
        ok = _close_enough(got, exp)
        assert ok.all(), (int((~ok).sum()), float(np.max(np.abs(got - exp))))
    assert np.unique(plain).size > 10000
    # a fixed sample against the oracle: every pair of two spliced sequences among the queries, and a pair inside every family (the first
    # seven) or across to it (the others: their members are candidates only)
    spliced = [i for i in range(NQ) if i % 9 == 4]
    sample = [(a, b) for a in spliced for b in spliced if a < b]
    sample += [(20 * f, 20 * f + 1) if 20 * f < NQ else ((7 * f + 3) % NQ, 20 * f + 1) for f in range(n // 20)]
    assert 130 <= len(sample) <= 160
    hist = {i: oracle.hist(seqs[i], 9, case["dtype"]) for i in sorted({i for p in sample for i in p})}
    for got, text in ((clamped, text3), (plain, _unclamped(text3))):
        model = oracle.predictor(text).reg
        for qi, ci in sample:
            want = min(max(oracle.score(model, hist[ci], hist[qi])[2], 0.0), 1.0)
            assert abs(got[qi, ci] - want) <= ATOL + RTOL * abs(want), (qi, ci, got[qi, ci], want)


def test_a_pairs_value_does_not_depend_on_the_call(ctx, case, plain):
    hs, n, q, pred = case["hs"], case["n"], case["q"], case["pred_lin"]
    # a permuted slot list: candidate indices are positions in it
    perm = np.random.default_rng(11).permutation(n).astype(np.uint32)
    got = _on(ctx, pred, hs, perm, hs, q)
    assert got[3]["route"] == api.PAIRS_ROUTE_MATRIX and got[3]["n_pairs"] == NQ * n
    assert np.array_equal(_bits(got[2].reshape(NQ, n)), _bits(plain[:, perm]))
    # windows per query, some empty, some with lo > hi
    rng = np.random.default_rng(12)
    lo = rng.integers(0, n, size=NQ).astype(np.uint64)
    hi = np.minimum(lo + rng.integers(1, 150, size=NQ), n + 5).astype(np.uint64)
    lo[::17] = hi[::17]
    lo[5::23] = hi[5::23] + 3
    got = _on(ctx, pred, hs, None, hs, q, win_lo=lo, win_hi=hi, m=n)
    assert got[3]["route"] == api.PAIRS_ROUTE_MATRIX
    listed = 0
    for j in range(NQ):
        a, b = int(got[0][j]), int(got[0][j + 1])
        w_lo, w_hi = int(min(lo[j], hi[j], n)), int(min(hi[j], n))
        assert np.array_equal(got[1][a:b], np.arange(w_lo, w_hi, dtype=np.uint32)), j
        assert np.array_equal(_bits(got[2][a:b]), _bits(plain[j, w_lo:w_hi])), j
        listed += b - a
    assert listed == got[3]["n_pairs"] > 0
    # 130 queries: blocks of 128 + 2 instead of 128 + 12
    got = _on(ctx, pred, hs, None, hs, q[:130], m=n)
    assert got[3]["route"] == api.PAIRS_ROUTE_MATRIX and got[3]["n_pairs"] == 130 * n
    assert np.array_equal(_bits(got[2].reshape(130, n)), _bits(plain[:130]))


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
pred = api.Predictor.from_text(ctx, weights_with_mode(_unclamped(_two_block(weights_text("weights_cfg5_k9.txt"))), 2))
ctx.set_pairs_div_cells(True)
q = np.arange(130, dtype=np.uint32)
one = pred.search_pairs(hs, None, hs, q, m=len(seqs))
assert one[3]["route"] == api.PAIRS_ROUTE_MATRIX and one[3]["n_pairs"] == q.size * len(seqs), one[3]
plain = one[2].reshape(q.size, len(seqs))
# 70 000 candidates (slots of the set, repeated): with 64 slices and 128 query rows the product array holds 65 536, so two chunks of 35 000 run
slots = np.random.default_rng(5).integers(0, len(seqs), size=70000).astype(np.uint32)
offsets, idx, sim, info = pred.search_pairs(hs, slots, hs, q)
assert info["route"] == api.PAIRS_ROUTE_MATRIX and info["n_pairs"] == q.size * slots.size, info
assert np.array_equal(idx.reshape(q.size, slots.size), np.broadcast_to(np.arange(slots.size, dtype=np.uint32), (q.size, slots.size)))
assert np.array_equal(sim.reshape(q.size, slots.size).view(np.uint64), np.ascontiguousarray(plain[:, slots]).view(np.uint64))
print("ok", info["n_pairs"])
"""


def test_candidates_in_several_chunks_give_the_same_bits():
    """MSC_GEMM_SLICES is read once per process: a child process, as test_candidates_in_several_chunks_keep_query_order does"""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MSC_GEMM_SLICES="64")
    r = subprocess.run([sys.executable, "-c", _CHUNKED, os.path.dirname(tests), tests], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"ok" in r.stdout, r.stdout.decode(errors="replace")[-3000:]


@pytest.mark.parametrize("why", ["groups_model", "k5_set", "k13_sparse", "one_query"])
def test_declines_keep_the_fallback(ctx, why):
    s, _ = synth.families(5150, 60, 1000, family=20)
    if why == "groups_model":
        hs, text = _set(ctx, s, 9, 8), GROUPS_TEXT
    elif why == "k5_set":
        hs, text = _set(ctx, s, 5, 16), weights_text("weights_k5_u16_slow.txt")
    elif why == "k13_sparse":
        hs, text = _set(ctx, s, 13, 64, sparse=True), weights_text("weights_cfg4_k13.txt")
    else:
        hs, text = _set(ctx, s, 9, 8), weights_text("weights_cfg5_k9.txt")
    pred = api.Predictor.from_text(ctx, text)
    q = np.arange(1 if why == "one_query" else 40, dtype=np.uint32)
    off = pred.search_pairs(hs, None, hs, q, m=len(s))
    got = _on(ctx, pred, hs, None, hs, q, m=len(s))
    assert off[3]["route"] == api.PAIRS_ROUTE_FALLBACK and got[3]["route"] == api.PAIRS_ROUTE_FALLBACK, (off[3], got[3])
    assert np.array_equal(got[0], off[0]) and np.array_equal(got[1], off[1]) and np.array_equal(_bits(got[2]), _bits(off[2]))


def test_switch_off_again_gives_the_parents_list(ctx, case):
    hs, n, q = case["hs"], case["n"], case["q"]
    on = _on(ctx, case["pred"], hs, None, hs, q, m=n)
    assert on[3]["route"] == api.PAIRS_ROUTE_MATRIX
    again = case["pred"].search_pairs(hs, None, hs, q, m=n)
    off = case["off"]
    assert again[3]["route"] == api.PAIRS_ROUTE_FALLBACK
    assert np.array_equal(again[0], off[0]) and np.array_equal(again[1], off[1]) and np.array_equal(_bits(again[2]), _bits(off[2]))


def test_fastcar_div_cells_writes_the_same_lines(tmp_path, seqs, text3):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "meshclust2_amd", "host", "msc_fastcar")
    db, qs = seqs[:60], [x[:len(x) - 5] for x in seqs[0:60:3]]          # 60 x 20, the queries relatives of the database's families
    synth.write_fasta(str(tmp_path / "db.fa"), db, [">seq%d" % i for i in range(len(db))])
    synth.write_fasta(str(tmp_path / "q.fa"), qs, [">qry%d" % i for i in range(len(qs))])
    with open(str(tmp_path / "w.txt"), "w") as f:
        f.write(text3)
    outs = []
    for extra in ([], ["--div-cells"]):
        prefix = "fc%d_" % len(extra)
        r = subprocess.run([exe, "db.fa", "--query", "q.fa", "--recover", "w.txt", "--output", prefix, "--kernels"] + extra, cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
        assert (b"divergence sums from cells" in r.stdout) == bool(extra), r.stdout.decode(errors="replace")[-2000:]
        outs.append([ln.split("\t") for ln in open(str(tmp_path / (prefix + "0"))).read().splitlines()])
    base, cells = outs
    assert len(base) == len(cells) > 20
    for a, b in zip(base, cells):
        assert a[:2] == b[:2] and len(a) == len(b) == 3
        assert abs(float(a[2]) - float(b[2])) <= 1e-9 * abs(float(a[2])), (a, b)          # (%g prints six digits)
