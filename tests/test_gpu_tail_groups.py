"""msc_set_tail_groups (default 8; csrc/msc_multi_plan.h): consecutive folded blocks of one query group of a msc_score_multi call
share ONE tail -- the bound screen, the listed pairs' exact counts, their walk and FP64 evaluation, the closing kernel, the close counts and the flags'
copy home run once for the group, blockIdx.y the block. Nothing a caller sees may change: the reference of every case is the same call under
set_tail_groups(0), on a model object of its own, and flags, counts, msc_last_fold_screen, msc_last_emd_walk, the kernel's name and its launches are
compared for equality. msc_last_tail_groups says what formed: (groups of two blocks and more, blocks in them).

A call's final groups halve down to one block (the ramp), so the short calls of a test form small groups; the context `flat` is made under
MSC_TAIL_NO_RAMP and keeps full groups to the end. The sets are those of tests/test_gpu_query_groups.py: 640 sequences of 1 kb in families of four,
k = 9, 32-bit, dense."""
import os

import numpy as np
import pytest

from golden_util import weights_text
from meshclust2_amd import api, synth
from test_gpu_fold_screen import _shifted, _w0
from test_gpu_query_groups import _built, _text, _with_runs

SEED, N, LEN, K, FAM = 20260002, 640, 1000, 9, 4
ORDERS = (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST)


@pytest.fixture(scope="module")
def seqs():
    return synth.families(SEED, N, LEN, family=FAM)[0]


@pytest.fixture(scope="module")
def ramped(seqs):
    """a context as it comes, and the set on it"""
    c = api.Context(0)
    yield dict(ctx=c, hs=_built(c, seqs))
    c.close()


@pytest.fixture(scope="module")
def flat(seqs):
    """a context made under MSC_TAIL_NO_RAMP (the library reads it when a context is made), and the set on it"""
    old = os.environ.get("MSC_TAIL_NO_RAMP")
    os.environ["MSC_TAIL_NO_RAMP"] = "1"
    try:
        c = api.Context(0)
    finally:
        if old is None:
            del os.environ["MSC_TAIL_NO_RAMP"]
        else:
            os.environ["MSC_TAIL_NO_RAMP"] = old
    yield dict(ctx=c, hs=_built(c, seqs))
    c.close()


def _call(ctx, cap, text, hs, cands, qs, order=api.ORDER_CAND_FIRST, m=None, qgroups=32, feat=None):
    """one flags-only call under set_tail_groups(cap), on a model of its own -> (result, everything else a caller can see of it, the tail groups it ran)"""
    feat = feat or api.Feature.from_text(ctx, text, 0)
    ctx.set_tail_groups(cap)
    ctx.set_query_groups(qgroups)
    try:
        got = api.score_multi(ctx, feat, hs, cands, hs, qs, order=order, m=m, want=("close", "counts"))
        return got, dict(fold=ctx.last_fold_screen(), walk=ctx.last_emd_walk(), kernel=ctx.last_kernel_info(), launches=ctx.last_kernel_launches()), ctx.last_tail_groups()
    finally:
        ctx.set_tail_groups(8)
        ctx.set_query_groups(32)


def _equal(got, ref, what):
    assert ref[2] == (0, 0), (what, ref[2])          # (the reference ran block by block)
    for name in ("close", "counts"):
        assert got[0][name].tobytes() == ref[0][name].tobytes(), (what, name)          # bit for bit
    assert got[1] == ref[1], (what, got[1], ref[1])


def _fp64(ctx, feat, hs, qs, m):
    ctx.set_fold_screen(0)
    try:
        full = api.score_multi(ctx, feat, hs, None, hs, qs, m=m, want=("sum", "close", "counts"))
    finally:
        ctx.set_fold_screen(16)
    assert np.array_equal(full["close"], (full["sum"] >= 0).astype(np.uint8))
    return full


QS680 = np.arange(680, dtype=np.uint32) % N          # 680 queries: five blocks of 128 and one of 40 (the last 40 are queries 0 .. 39 again)


@pytest.mark.gpu
@pytest.mark.parametrize("which,cap,formed", [("flat", 2, (2, 4)), ("flat", 8, (1, 5)), ("ramped", 2, (2, 4)), ("ramped", 8, (2, 4))])
def test_five_blocks_and_a_short_one(request, which, cap, formed):
    """five blocks of 128 and one of 40 rows, cap 2 and cap 8, both argument orders, a shuffled candidate slot list and m = 601 without a list: the
    reference's flags, counts and counters; all six blocks folded, none fell back; the block of 40 rows is in no group. Without the ramp cap 2 forms
    two pairs and leaves a block alone, cap 8 one group of five; with it six blocks are cut 2, 2, 1, 1 under either cap."""
    w = request.getfixturevalue(which)
    ctx, hs, text = w["ctx"], w["hs"], _text()
    rng = np.random.default_rng(11)
    for order in ORDERS:
        for cands, m in ((rng.permutation(N).astype(np.uint32), None), (None, 601)):
            ref = _call(ctx, 0, text, hs, cands, QS680, order, m)
            got = _call(ctx, cap, text, hs, cands, QS680, order, m)
            print("%s cap %d order %d m %s: %r, tail groups %r" % (which, cap, order, m, got[1], got[2]))
            _equal(got, ref, (which, cap, order, m))
            assert got[1]["fold"] == (16, 6, 0) and got[1]["walk"][2] == 6 and got[1]["walk"][0] > 0
            assert got[2] == formed


@pytest.mark.gpu
def test_tail_groups_stop_at_the_query_groups_ends(flat):
    """the same call under set_query_groups(2) with tail cap 8: query groups of two, so tail groups of two and the fifth block alone; under
    set_query_groups(0) no tail group forms; the results are the reference's"""
    ctx, hs, text = flat["ctx"], flat["hs"], _text()
    ref = _call(ctx, 0, text, hs, None, QS680, m=N)
    for qgroups, formed in ((2, (2, 4)), (0, (0, 0)), (1, (0, 0)), (32, (1, 5))):
        got = _call(ctx, 8, text, hs, None, QS680, m=N, qgroups=qgroups)
        print("query groups %d: tail groups %r" % (qgroups, got[2]))
        _equal(got, ref, qgroups)
        assert got[2] == formed and got[1]["fold"] == (16, 6, 0)


@pytest.mark.gpu
def test_overflowing_blocks_of_a_group_run_again(flat, seqs):
    """a 400-base run in every ninth sequence, 300 queries, cap 2: one group of two and a short block. The blocks whose list overflows, and only those,
    are scored again -- the counters are the reference's -- and the flags are the FP64 flags"""
    ctx, text = flat["ctx"], _text()
    hs = _built(ctx, _with_runs(seqs, 9))
    qs = np.arange(300, dtype=np.uint32)
    ref = _call(ctx, 0, text, hs, None, qs, m=N)
    got = _call(ctx, 2, text, hs, None, qs, m=N)
    print("runs in every ninth: %r, tail groups %r" % (got[1], got[2]))
    _equal(got, ref, "runs")
    assert got[1]["fold"][:2] == (16, 3) and got[2] == (1, 2)
    full = _fp64(ctx, api.Feature.from_text(ctx, text, 0), hs, qs, N)
    assert np.array_equal(got[0]["close"], full["close"]) and np.array_equal(got[0]["counts"], full["counts"])


@pytest.mark.gpu
def test_threshold_through_the_listed_pairs_of_a_group(flat):
    """the intercept moved by the median FP64 sum of the related pairs, 384 queries in one group of three: the grouped list kernels (exact counts, walk,
    FP64 evaluation) decide the related pairs' flags, which are the FP64 flags"""
    ctx, hs, text = flat["ctx"], flat["hs"], _text()
    qs = np.arange(384, dtype=np.uint32)
    related = (np.arange(N)[None, :] // FAM) == (qs[:, None] // FAM)
    sums = _fp64(ctx, api.Feature.from_text(ctx, text, 0), hs, qs, N)["sum"]
    moved = _shifted(text, _w0(text) - float(np.median(sums[related])))
    full = _fp64(ctx, api.Feature.from_text(ctx, moved, 0), hs, qs, N)
    assert 0.3 < float(full["close"][related].mean()) < 0.7          # the boundary really runs through them
    ref = _call(ctx, 0, moved, hs, None, qs, m=N)
    got = _call(ctx, 8, moved, hs, None, qs, m=N)
    print("moved: %r, tail groups %r" % (got[1], got[2]))
    _equal(got, ref, "moved")
    assert got[2] == (1, 3) and got[1]["fold"] == (16, 3, 0) and got[1]["walk"][0] > 0
    assert np.array_equal(got[0]["close"], full["close"]) and np.array_equal(got[0]["counts"], full["counts"])


@pytest.mark.gpu
def test_sixteen_bit_bins_at_k_8(flat, seqs):
    """a 16-bit set at k = 8 with the k = 8 weights, 384 queries in one group of three: the reference's flags, counts and counters"""
    ctx = flat["ctx"]
    hs = _built(ctx, seqs, 8, 16)
    text = weights_text("weights_k8_u16.txt")
    qs = np.arange(384, dtype=np.uint32)
    ref = _call(ctx, 0, text, hs, None, qs, m=N)
    got = _call(ctx, 8, text, hs, None, qs, m=N)
    print("k 8: %r, tail groups %r" % (got[1], got[2]))
    _equal(got, ref, "k 8")
    assert got[1]["fold"][:2] == (16, 3) and got[2] == (1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [129, 256])
def test_calls_too_short_for_a_group(ramped, nq):
    """129 queries (a block of 128 and one of one row) and 256 queries (two blocks, which the ramp leaves alone): nothing forms, the result is unchanged"""
    ctx, hs, text = ramped["ctx"], ramped["hs"], _text()
    qs = np.arange(nq, dtype=np.uint32)
    ref = _call(ctx, 0, text, hs, None, qs, m=N)
    got = _call(ctx, 8, text, hs, None, qs, m=N)
    _equal(got, ref, nq)
    assert got[2] == (0, 0)
