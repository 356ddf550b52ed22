"""msc_set_fold_screen (default 16; csrc/msc_fold.h): the close-flag blocks of msc_score_multi that take the bounds of the
earth mover's distance run their matrix product over presence bits folded F-to-1. The product then gives upper bounds of the two sums it
used to give exactly (P1 <= P1' + min(x_q, x_c), P2 <= P2'; lower bounds 0), the screen evaluates every statistic over the intervals, and
the pairs it leaves open -- every related pair among them -- get their exact counts one by one (k_fold_exact_list) before the FP64
evaluation. A block whose list overflows is scored again with the true product. Whatever a block takes, its flags must be those of the FP64
evaluation of every pair: "FP64 flags" below is the same call with the switch off and want=("sum", "close", "counts"), which evaluates
every pair in FP64. msc_last_fold_screen says what ran: (fold, folded blocks, blocks that fell back).

The sets are 640 sequences in families of FOUR: related pairs are always listed, 3 of 640 candidates = 0.47 % of a block against a list of
1/64 = 1.56 %; families of 20 would overflow every block (tests/test_gpu_emd_bounds.py's set does, and falls back).
The public call has no first slot: a run of slots that does not start at 0 is given as a slot list (39 .. 639, m = 601), and m = 601
without a list is slots 0 .. 600."""
import numpy as np
import pytest

from golden_util import weights_text
from meshclust2_amd import api, synth

SEED, N, LEN, K, NQ, FAM = 20260002, 640, 1000, 9, 200, 4
ORDERS = (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST)


def _text(k=9, dtype=32):
    return weights_text("weights_k9_u32.txt").replace("k: 9", "k: %d" % k).replace("uint32_t", "uint%d_t" % dtype)


def _w0(text):
    lines = text.splitlines()
    return float(lines[next(i for i, ln in enumerate(lines) if ln.startswith("n_combos:")) + 1])


def _shifted(text, w0):
    """the classification block of a weights file with its intercept replaced (the line after the first `n_combos:`)"""
    lines = text.splitlines()
    lines[next(i for i, ln in enumerate(lines) if ln.startswith("n_combos:")) + 1] = repr(float(w0))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seqs():
    return synth.families(SEED, N, LEN, family=FAM)[0]


def _fp64(ctx, feat, hs, cands, qset, qs, order=api.ORDER_CAND_FIRST, m=None):
    ctx.set_fold_screen(0)
    try:
        full = api.score_multi(ctx, feat, hs, cands, qset, qs, order=order, m=m, want=("sum", "close", "counts"))
    finally:
        ctx.set_fold_screen(16)
    assert np.array_equal(full["close"], (full["sum"] >= 0).astype(np.uint8))
    return full


def _flags(ctx, feat, hs, cands, qset, qs, order=api.ORDER_CAND_FIRST, m=None, fold=16):
    """the close-flag-only call under msc_set_fold_screen(fold) -> (result, (fold, folded, fell_back), (listed, dense, blocks), kernel name)"""
    ctx.set_fold_screen(fold)
    try:
        got = api.score_multi(ctx, feat, hs, cands, qset, qs, order=order, m=m, want=("close", "counts"))
        return got, ctx.last_fold_screen(), ctx.last_emd_walk(), ctx.last_kernel_info()[0]
    finally:
        ctx.set_fold_screen(16)


@pytest.fixture(scope="module")
def world(ctx, seqs):
    """the dense 32-bit set at k = 9, its model and the FP64 evaluation of the 200 x 640 block in both argument orders, computed once"""
    hs = api.HistogramSet(ctx, K, 32, N)
    for off in range(0, N, 256):
        hs.build(seqs[off:off + 256], first_slot=off)
    text = _text()
    feat = api.Feature.from_text(ctx, text, 0)
    qs = np.arange(NQ, dtype=np.uint32)
    full = {o: _fp64(ctx, feat, hs, None, hs, qs, o, m=N) for o in ORDERS}
    related = (np.arange(N)[None, :] // FAM) == (qs[:, None] // FAM)
    return dict(hs=hs, text=text, feat=feat, qs=qs, full=full, related=related)


def _same(got, full, cols=None):
    want = full["close"] if cols is None else full["close"][:, cols]
    assert np.array_equal(got["close"], want)
    assert np.array_equal(got["counts"], want.sum(axis=1).astype(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_common_path(ctx, world, order):
    """200 queries = two blocks (128 and 72 rows), a shuffled slot list, the run of slots 39 .. 639 (m = 601) and m = 601 without a list: the
    FP64 flags, both blocks folded, none fell back, pairs listed; and the switch off gives the same flags with nothing folded"""
    hs, feat, qs, full = world["hs"], world["feat"], world["qs"], world["full"][order]
    rng = np.random.default_rng(7)
    for cands, m in ((rng.permutation(N).astype(np.uint32), None), (np.arange(39, N, dtype=np.uint32), None), (None, 601)):
        cols = cands if cands is not None else np.arange(m)
        got, fold, walk, name = _flags(ctx, feat, hs, cands, hs, qs, order, m=m)
        print("order %d m %d: fold %r, walk %r, %s" % (order, cols.size, fold, walk, name))
        _same(got, full, cols)
        assert fold == (16, 2, 0) and walk[0] > 0 and walk[1] == 0 and walk[2] == 2
        assert name.startswith("k_pair_gemm_fp4_dma") and "folded x 16" in name
        assert walk[0] <= 128 * cols.size // 64 + 72 * cols.size // 64
    off, fold, walk, name = _flags(ctx, feat, hs, None, hs, qs, order, m=N, fold=0)
    _same(off, full)
    assert fold == (0, 0, 0) and "folded" not in name and walk[1] == 0 and walk[2] == 2


@pytest.mark.gpu
def test_a_few_rows_against_the_oracle(ctx, seqs, world):
    """three query rows against 200 candidates: the oracle's get_close flags (candidate first, a length window that admits everything)"""
    from oracle import oracle_py
    pred = oracle_py.predictor(world["text"])
    oh = [oracle_py.hist(s, K, 32) for s in seqs[:200]]
    rows = np.array([3, 129, 130], dtype=np.uint32)
    feat = api.Feature.from_text(ctx, world["text"], 0)          # (a model of its own: a call whose small list overflows is remembered on the model)
    got, fold, walk, _ = _flags(ctx, feat, world["hs"], None, world["hs"], rows, m=200)
    assert fold[:2] == (16, 1)          # (9 related pairs fill this small block's list of 600 / 64 = 9: it may fall back)
    for i, q in enumerate(rows):
        f = oracle_py.get_close(pred, 1e-9, oh[int(q)], oh)[0]
        assert np.array_equal(got["close"][i], f), q
    for h in oh:
        oracle_py.lib().orc_hist_free(h)


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [8, 32])
def test_other_folds(ctx, world, fold):
    got, used, walk, name = _flags(ctx, world["feat"], world["hs"], None, world["hs"], world["qs"], m=N, fold=fold)
    print("fold %d: %r, walk %r" % (fold, used, walk))
    _same(got, world["full"][api.ORDER_CAND_FIRST])
    assert used[0] == fold and used[1] == 2 and "folded x %d" % fold in name
    if fold == 8:
        assert used[2] == 0 and walk[0] > 0


@pytest.mark.gpu
def test_sparse_mirrors(ctx, seqs, world):
    """the same sequences as a SPARSE set (mirrors built from the lists, msc_set_sparse_matrix_pass): the dense set's FP64 flags"""
    sp = api.HistogramSet(ctx, K, 32, N, sparse_entries=sum(len(s) for s in seqs) + 1024)
    sp.build(seqs)
    ctx.set_sparse_matrix_pass(True)
    try:
        for order in ORDERS:
            got, fold, walk, name = _flags(ctx, world["feat"], sp, None, sp, world["qs"], order, m=N)
            print("sparse, order %d: fold %r, walk %r, %s" % (order, fold, walk, name))
            _same(got, world["full"][order])
            assert fold == (16, 2, 0) and walk[0] > 0 and "mirrors from lists" in name
    finally:
        ctx.set_sparse_matrix_pass(False)


@pytest.mark.gpu
def test_sixteen_bit_set_at_k8(ctx, seqs):
    hs = api.HistogramSet(ctx, 8, 16, N)
    hs.build(seqs)
    feat = api.Feature.from_text(ctx, weights_text("weights_k8_u16.txt"), 0)
    qs = np.arange(NQ, dtype=np.uint32)
    for order in ORDERS:
        full = _fp64(ctx, feat, hs, None, hs, qs, order, m=N)
        got, fold, walk, name = _flags(ctx, feat, hs, None, hs, qs, order, m=N)
        print("k 8, 16-bit, order %d: fold %r, walk %r" % (order, fold, walk))
        _same(got, full)
        assert fold[0] == 16 and fold[1] == 2


@pytest.mark.gpu
def test_a_k5_set_is_never_folded(ctx):
    """1 024 bins: 4^k / 8 is less than a super-step of the product; the set keeps the true product and returns the same flags"""
    short = synth.families(77, 300, 200, family=FAM)[0]
    hs = api.HistogramSet(ctx, 5, 32, len(short))
    hs.build(short)
    feat = api.Feature.from_text(ctx, _text(5, 32), 0)
    qs = np.arange(150, dtype=np.uint32)
    full = _fp64(ctx, feat, hs, None, hs, qs, m=len(short))
    for f in (8, 16, 32):
        got, fold, walk, name = _flags(ctx, feat, hs, None, hs, qs, m=len(short), fold=f)
        _same(got, full)
        assert fold == (0, 0, 0) and "folded" not in name


def _moved(ctx, world_text, by):
    return api.Feature.from_text(ctx, _shifted(world_text, _w0(world_text) - float(by)), 0)


@pytest.mark.gpu
def test_threshold_through_the_listed_pairs(ctx, world):
    """the intercept moved by the median FP64 sum of the related pairs: the exact counts of k_fold_exact_list decide their flags"""
    hs, qs, rel = world["hs"], world["qs"], world["related"]
    sums = world["full"][api.ORDER_CAND_FIRST]["sum"]
    moved = _moved(ctx, world["text"], np.median(sums[rel]))
    full = _fp64(ctx, moved, hs, None, hs, qs, m=N)
    assert 0.3 < float(full["close"][rel].mean()) < 0.7          # the boundary really runs through them
    got, fold, walk, _ = _flags(ctx, moved, hs, None, hs, qs, m=N)
    print("fold %r, walk %r" % (fold, walk))
    _same(got, full)
    assert fold == (16, 2, 0) and walk[0] > 0


@pytest.mark.gpu
def test_threshold_beside_the_unrelated_bulk(ctx, world):
    """s = 0 put 0.25 above the largest FP64 sum of an unrelated pair: the intervals of the bulk reach towards the threshold; the counter is
    reported, not asserted (on an MI355X: see profiles/fold_screen.md)"""
    hs, qs, rel = world["hs"], world["qs"], world["related"]
    sums = world["full"][api.ORDER_CAND_FIRST]["sum"]
    moved = _moved(ctx, world["text"], float(sums[~rel].max()) + 0.25)
    full = _fp64(ctx, moved, hs, None, hs, qs, m=N)
    assert not full["close"][~rel].any()
    got, fold, walk, _ = _flags(ctx, moved, hs, None, hs, qs, m=N)
    print("beside the bulk: fold %r, walk %r" % (fold, walk))
    _same(got, full)


@pytest.mark.gpu
def test_overflow_falls_back_and_the_model_remembers(ctx, world):
    """the intercept moved by the median sum of ALL pairs: every block's folded list overflows and the block is scored again with the true product (whose
    list overflows too: the dense walk produces the flags); the same model object then takes the unfolded route"""
    hs, qs = world["hs"], world["qs"]
    sums = world["full"][api.ORDER_CAND_FIRST]["sum"]
    moved = _moved(ctx, world["text"], np.median(sums))
    full = _fp64(ctx, moved, hs, None, hs, qs, m=N)
    assert 0.45 < float(full["close"].mean()) < 0.55
    got, fold, walk, _ = _flags(ctx, moved, hs, None, hs, qs, m=N)
    print("first call: fold %r, walk %r" % (fold, walk))
    _same(got, full)
    assert fold == (16, 2, 2)
    again, fold, walk, name = _flags(ctx, moved, hs, None, hs, qs, m=N)
    print("second call: fold %r, walk %r" % (fold, walk))
    _same(again, full)
    assert fold == (0, 0, 0) and "folded" not in name


def _kmer_bins(codes, k):
    """the distinct k-mer bins of a sequence of 0..3 codes, first base most significant"""
    c = codes.astype(np.int64)
    b = np.zeros(c.size - k + 1, dtype=np.int64)
    for i in range(k):
        b = b * 4 + c[i:c.size - k + 1 + i]
    return np.unique(b)


@pytest.mark.gpu
def test_a_set_built_to_collide(ctx):
    """Each sequence is two copies of its template that differ at every 9th base (members 0.5 % substitutions and 0.2 % indels apart: at the
    3 % of the other sets the related pairs share half their k-mers, and what the folded count loses to collisions it regains from chance
    matches among the other half). msc_fold_bin drops the FIRST digits of a bin (F = 16: the
    first two bases of a 9-mer), and every window of 9 bases of the second copy holds exactly one changed base: where it is one of the first
    two, the window's k-mer and the first copy's fall into one folded bin. A related pair shares both, so its OR-folded shared count is far
    below the true one -- without the slots' own collisions x the upper bound of P1 would be wrong. Asserted on the CPU first, then the
    three intercepts of the tests above."""
    n, nq, half = 320, 160, 500
    codes = []
    for t in range(n // FAM):
        tmpl = synth.template(911, t, half)
        second = tmpl.copy()
        second[4::9] = (second[4::9] + 1) & 3
        both = np.concatenate([tmpl, second])
        codes += [synth.member(911, t, j, both, sub_rate=0.005, indel_rate=0.002) for j in range(FAM)]
    nbins = 4 ** K
    bins = [_kmer_bins(c, K) for c in codes]
    every = np.unique(np.concatenate(bins))
    fmap = dict(zip(every.tolist(), (api.fold_bin(b, nbins, 16) for b in every.tolist())))
    folded = [np.unique(np.array([fmap[x] for x in b.tolist()], dtype=np.int64)) for b in bins]
    short = 0
    for a in range(n):
        for b in range(a + 1, (a // FAM + 1) * FAM):
            true = np.intersect1d(bins[a], bins[b]).size
            short += int(true - np.intersect1d(folded[a], folded[b]).size >= 20)
    print("related pairs whose OR-folded shared count is 20 or more below the true one: %d of %d" % (short, n // FAM * 6))
    assert short >= 50
    seqs = [synth.to_ascii(c) for c in codes]
    hs = api.HistogramSet(ctx, K, 32, n)
    hs.build(seqs)
    text = _text()
    feat = api.Feature.from_text(ctx, text, 0)
    qs = np.arange(nq, dtype=np.uint32)
    rel = (np.arange(n)[None, :] // FAM) == (qs[:, None] // FAM)
    base = _fp64(ctx, feat, hs, None, hs, qs, m=n)
    got, fold, walk, _ = _flags(ctx, feat, hs, None, hs, qs, m=n)
    print("as trained: fold %r, walk %r" % (fold, walk))
    _same(got, base)
    assert fold[:2] == (16, 2)
    sums = base["sum"]
    for what, by in (("related median", np.median(sums[rel])), ("beside the bulk", float(sums[~rel].max()) + 0.25), ("median of all", np.median(sums))):
        moved = _moved(ctx, text, by)
        full = _fp64(ctx, moved, hs, None, hs, qs, m=n)
        got, fold, walk, _ = _flags(ctx, moved, hs, None, hs, qs, m=n)
        print("%s: fold %r, walk %r, close %.3f" % (what, fold, walk, float(full["close"].mean())))
        _same(got, full)


@pytest.mark.gpu
@pytest.mark.parametrize("every", [9, 40])
def test_repeat_bearing_queries(ctx, seqs, every):
    """a 400-base homopolymer in place of 400 bases of every ninth sequence (as test_thirty_two_bit_ranks of tests/test_gpu_emd_bounds.py): large
    bins on both sides -- the hot list by folded bin, P2', and the exact P2 of the listed pairs. A repeat-bearing query leaves every
    candidate open that holds the repeat's FOLDED bin (P2' = 391 there), about 6 % of them, and every pair of two repeat-bearing sequences is
    open: with every ninth sequence bearing one, 1.2 % + 0.7 % of a block on top of the related 0.6 % pass the list's 1.56 % and the blocks
    fall back (reported); with every 40th -- 0.06 % + 0.15 % -- they do not, and the listed pairs' exact P2 decide."""
    rep = []
    for i, s in enumerate(seqs):
        s = bytes(s)
        if i % every == 1:
            at = 100 + 13 * (i % 40)
            s = s[:at] + b"A" * 400 + s[at + 400:]
        rep.append(s)
    hs = api.HistogramSet(ctx, K, 32, len(rep))
    hs.build(rep)
    qs = np.arange(NQ, dtype=np.uint32)
    for order in ORDERS:
        feat = api.Feature.from_text(ctx, _text(), 0)          # (a model per call: one whose blocks fell back is remembered)
        full = _fp64(ctx, feat, hs, None, hs, qs, order, m=len(rep))
        got, fold, walk, _ = _flags(ctx, feat, hs, None, hs, qs, order, m=len(rep))
        print("every %d, order %d: fold %r, walk %r" % (every, order, fold, walk))
        _same(got, full)
        assert fold[:2] == (16, 2)
        if every == 40:
            assert fold[2] == 0 and walk[0] > 0
