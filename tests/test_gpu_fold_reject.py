"""msc_set_fold_reject (default on; csrc/msc_fold_reject.h): a folded block of msc_score_multi proves an integer cut T(q) per query row
once -- every candidate within the ranges of its set whose folded product output P1' + P2' is at most T(q) is not close -- and its screen evaluates only
the waves of 64 queries x 1 candidate that hold a pair above the cut or a row without one. Whatever the cut does, the flags must be those of the FP64
evaluation of every pair (MSC_NO_SCREEN's path: the same call with the folded screen off and want=("sum", "close", "counts")) and those of the switch
off. msc_last_fold_reject says what it did: (pairs rejected, query rows without a cut).

The sets are tests/test_gpu_fold_screen.py's: 640 sequences in families of four, related pairs 0.47 % of a block."""
import os

import numpy as np
import pytest

from golden_util import weights_text
from meshclust2_amd import api, synth

SEED, N, LEN, K, FAM = 20260002, 640, 1000, 9, 4
ORDERS = (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST)


def _text(k=9, dtype=32, name="weights_k9_u32.txt"):
    return re_k(weights_text(name), k, dtype)


def re_k(text, k, dtype):
    lines = text.splitlines()
    lines = ["k: %d" % k if ln.startswith("k:") else "Datatype: uint%d_t" % dtype if ln.startswith("Datatype:") else ln for ln in lines]
    return "\n".join(lines) + "\n"


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


def _flags(ctx, feat, hs, cands, qset, qs, order=api.ORDER_CAND_FIRST, m=None, reject=True):
    """the close-flag-only call with the cut on or off -> (result, (rejected, rows without a cut), (fold, folded, fell_back), (listed, dense, blocks))"""
    ctx.set_fold_reject(reject)
    try:
        got = api.score_multi(ctx, feat, hs, cands, qset, qs, order=order, m=m, want=("close", "counts"))
        return got, ctx.last_fold_reject(), ctx.last_fold_screen(), ctx.last_emd_walk()
    finally:
        ctx.set_fold_reject(True)


def _same(got, full, cols=None):
    want = full["close"] if cols is None else full["close"][:, cols]
    assert np.array_equal(got["close"], want)
    assert np.array_equal(got["counts"], want.sum(axis=1).astype(np.uint64))


def _both(ctx, feat, hs, cands, qset, qs, full, order=api.ORDER_CAND_FIRST, m=None, cols=None, what=""):
    """on and off against the FP64 flags and one another; -> (counters on, fold on, walk on, walk off)"""
    on, rej, fold, walk = _flags(ctx, feat, hs, cands, qset, qs, order, m)
    off, rej_off, fold_off, walk_off = _flags(ctx, feat, hs, cands, qset, qs, order, m, reject=False)
    print("%s order %d: reject %r, fold %r, walk %r (off: fold %r, walk %r)" % (what, order, rej, fold, walk, fold_off, walk_off))
    _same(on, full, cols)
    _same(off, full, cols)
    assert np.array_equal(on["close"], off["close"]) and np.array_equal(on["counts"], off["counts"])
    assert rej_off == (0, 0)
    return rej, fold, walk, walk_off


@pytest.fixture(scope="module")
def world(ctx, seqs):
    """the dense 32-bit set at k = 9, its model and the FP64 evaluation of 130 x 640 in both argument orders, computed once"""
    hs = api.HistogramSet(ctx, K, 32, N)
    for off in range(0, N, 256):
        hs.build(seqs[off:off + 256], first_slot=off)
    text = _text()
    feat = api.Feature.from_text(ctx, text, 0)
    qs = np.arange(130, dtype=np.uint32)
    full = {o: _fp64(ctx, feat, hs, None, hs, qs, o, m=N) for o in ORDERS}
    related = (np.arange(N)[None, :] // FAM) == (qs[:, None] // FAM)
    return dict(hs=hs, text=text, feat=feat, qs=qs, full=full, related=related)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_common_path(ctx, world, order):
    """130 queries (a full block and one of 2 rows) x 639 candidates -- the last chunk of four is short --, contiguous and as a shuffled slot list: the FP64
    flags, the flags and counts of the switch off, pairs rejected, and no more pairs listed than without the cut"""
    hs, feat, qs, full = world["hs"], world["feat"], world["qs"], world["full"][order]
    rng = np.random.default_rng(11)
    shuffled = rng.permutation(N).astype(np.uint32)[:639]
    for cands, m in ((None, 639), (shuffled, None)):
        cols = cands if cands is not None else np.arange(m)
        rej, fold, walk, walk_off = _both(ctx, feat, hs, cands, hs, qs, full, order, m, cols, "k 9, 32-bit, m %d" % cols.size)
        assert fold == (16, 2, 0)
        assert rej[0] > 0 and rej[0] <= 130 * 639
        assert 0 < walk[0] <= walk_off[0]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_sixteen_bit_set_at_k8(ctx, seqs, order):
    """k = 8, 16-bit bins, the golden k = 8 model with its intercept moved by -2 (as trained it calls every pair of this set close: no row can have a cut)"""
    hs = api.HistogramSet(ctx, 8, 16, N)
    hs.build(seqs)
    text = weights_text("weights_k8_u16.txt")
    feat = api.Feature.from_text(ctx, _shifted(text, _w0(text) - 2.0), 0)
    qs = np.arange(130, dtype=np.uint32)
    full = _fp64(ctx, feat, hs, None, hs, qs, order, m=639)
    assert full["close"].any() and not full["close"].all()
    rng = np.random.default_rng(12)
    for cands, m in ((None, 639), (rng.permutation(N).astype(np.uint32)[:639], None)):
        ref = full if cands is None else _fp64(ctx, feat, hs, cands, hs, qs, order)
        rej, fold, walk, walk_off = _both(ctx, feat, hs, cands, hs, qs, ref, order, m, None, "k 8, 16-bit")
        assert fold == (16, 2, 0)
        assert rej[0] > 0 and 0 < walk[0] <= walk_off[0]


@pytest.mark.gpu
def test_a_wave_that_holds_a_related_pair(ctx, world):
    """64 queries x 1 candidate is a wave: with queries 0 .. 127 in slot order the family of candidate c sits in lanes c % 64 .. -- candidates 0 .. 3 put a
    related pair in lane 0, candidates 60 .. 63 one in lane 63; and with the queries rotated by one, a family straddles two waves. All 64 lanes of such a
    wave are evaluated: flags equal"""
    hs, feat = world["hs"], world["feat"]
    for qs in (np.arange(128, dtype=np.uint32), np.roll(np.arange(128, dtype=np.uint32), 1), np.arange(63, 63 + 128, dtype=np.uint32)):
        full = _fp64(ctx, feat, hs, None, hs, qs, m=N)
        rel = (np.arange(N)[None, :] // FAM) == (qs[:, None] // FAM)
        assert rel[0].any() and rel[63].any()
        rej, fold, walk, _ = _both(ctx, feat, hs, None, hs, qs, full, m=N, what="lanes")
        assert rej[0] > 0 and full["close"][rel].any()
        # every pair of a wave that holds a related pair was evaluated: at most the other waves' pairs were rejected
        waves_with_related = sum(int(rel[g * 64:(g + 1) * 64, c].any()) for g in range(2) for c in range(N))
        assert rej[0] <= (2 * N - waves_with_related) * 64


def _moved(ctx, text, by):
    return api.Feature.from_text(ctx, _shifted(text, _w0(text) - float(by)), 0)


@pytest.mark.gpu
def test_threshold_moved(ctx, world):
    """the intercept moved so that s = 0 lies 0.25 above the largest FP64 sum of an unrelated pair (test_threshold_beside_the_unrelated_bulk's construction) and
    by the median sum of the related pairs: small cuts or none, and the FP64 flags"""
    hs, qs, rel = world["hs"], world["qs"], world["related"]
    sums = world["full"][api.ORDER_CAND_FIRST]["sum"]
    for what, by in (("beside the bulk", float(sums[~rel].max()) + 0.25), ("through the listed pairs", float(np.median(sums[rel])))):
        moved = _moved(ctx, world["text"], by)
        full = _fp64(ctx, moved, hs, None, hs, qs, m=N)
        rej, fold, walk, _ = _both(ctx, moved, hs, None, hs, qs, full, m=N, what=what)
        assert rej[0] + rej[1] * N <= qs.size * N


@pytest.mark.gpu
def test_wide_ranges(ctx):
    """lengths 300 .. 3 000: either no row gets a cut or those that do are right"""
    codes, _ = synth.family_codes(31, 320, 1650, family=FAM, length_jitter=1350)
    lens = sorted({c.size for c in codes})
    assert lens[0] < 700 and lens[-1] > 2500
    seqs = [synth.to_ascii(c) for c in codes]
    hs = api.HistogramSet(ctx, K, 32, len(seqs))
    hs.build(seqs)
    feat = api.Feature.from_text(ctx, _text(), 0)
    qs = np.arange(130, dtype=np.uint32)
    for order in ORDERS:
        full = _fp64(ctx, feat, hs, None, hs, qs, order, m=len(seqs))
        rej, fold, walk, _ = _both(ctx, feat, hs, None, hs, qs, full, order, m=len(seqs), what="lengths %d..%d" % (lens[0], lens[-1]))
        assert rej[1] <= qs.size and rej[0] <= (qs.size - rej[1]) * len(seqs)


@pytest.mark.gpu
def test_similarity_ratio_across_a_wrap(ctx, seqs):
    """32-bit bins and a model that holds similarity_ratio, whose 32-bit form wraps once per pair unless the SECOND argument has no bin above the first's
    (neg = 0). Eight queries of 16 bases in a query set of their own: 8 k-mers, fewer than the sum of minima the fold and the candidates' lists allow -- with
    the candidate first, neg = 0 lies in such a row's box beside the neg >= 1 of every real pair, the box straddles a wrap, and the row gets no cut. The
    122 ordinary rows beside them get theirs."""
    short = [bytes(s)[100:116] for s in seqs[:8]]
    hs = api.HistogramSet(ctx, K, 32, 320)
    hs.build(list(seqs[:320]))
    queries = short + [bytes(s) for s in seqs[320:442]]
    qset = api.HistogramSet(ctx, K, 32, len(queries))
    qset.build(queries)
    feat = api.Feature.from_text(ctx, _text(), 0)
    assert (1 << 28) in [int(ln.split()[0]) for ln in _text().split("n_singles:")[1].splitlines()[1:7]]
    qs = np.arange(len(queries), dtype=np.uint32)
    for order in ORDERS:
        full = _fp64(ctx, feat, hs, None, qset, qs, order, m=320)
        rej, fold, walk, _ = _both(ctx, feat, hs, None, qset, qs, full, order, m=320, what="wrap")
        assert fold == (16, 2, 0) and rej[0] > 0
        if order == api.ORDER_CAND_FIRST:          # (query first, the second argument is the candidate: its excess is far above what the cut lets the sum of minima reach)
            assert 8 <= rej[1] < qs.size


@pytest.mark.gpu
def test_a_zero_length_sequence_among_the_candidates(ctx, seqs):
    """one empty sequence among the candidates: length_difference throws for its pairs, and the call fails with the cut as without it. The cut must not
    have swallowed the error: a zero length in range leaves every row without a cut (tests/fold_reject_check.cpp holds the header to that), so the pairs
    of the empty candidate are evaluated and reported as they always were. The same set without the empty slot among the candidates (m one less) is
    scored, the empty slot still in the set's ranges: the call succeeds, no row has a cut, nothing is rejected"""
    alls = list(seqs[:319]) + [b""]
    hs = api.HistogramSet(ctx, K, 32, len(alls))
    hs.build(alls)
    qs = np.arange(130, dtype=np.uint32)
    for reject in (True, False):
        feat = api.Feature.from_text(ctx, _text(), 0)
        ctx.set_fold_reject(reject)
        try:
            with pytest.raises(Exception):
                api.score_multi(ctx, feat, hs, None, hs, qs, m=len(alls), want=("close", "counts"))
        finally:
            ctx.set_fold_reject(True)
    feat = api.Feature.from_text(ctx, _text(), 0)
    full = _fp64(ctx, feat, hs, None, hs, qs, m=319)
    rej, fold, walk, _ = _both(ctx, feat, hs, None, hs, qs, full, m=319, what="zero length in the set's ranges")
    assert fold == (16, 2, 0) and rej == (0, qs.size)


@pytest.mark.gpu
def test_a_longer_sequence_arrives(ctx, seqs):
    """a set is scored, then a 3 000-base sequence is written into a spare slot: the ranks mirror is laid out again at a longer pitch, every slot's rank
    moment changes with it, and the ranges behind the cut must be taken again -- the flags of the second call are the FP64 path's"""
    hs = api.HistogramSet(ctx, K, 32, 321)
    hs.build(list(seqs[:320]))
    feat = api.Feature.from_text(ctx, _text(), 0)
    qs = np.arange(130, dtype=np.uint32)
    full = _fp64(ctx, feat, hs, None, hs, qs, m=320)
    rej, fold, walk, _ = _both(ctx, feat, hs, None, hs, qs, full, m=320, what="before")
    assert fold == (16, 2, 0) and rej[0] > 0
    long_one = synth.families(5, 1, 3000, family=1)[0][0]
    hs.build([long_one], first_slot=320)
    qs2 = np.concatenate([[320], np.arange(129)]).astype(np.uint32)
    for order in ORDERS:
        feat = api.Feature.from_text(ctx, _text(), 0)
        full = _fp64(ctx, feat, hs, None, hs, qs2, order, m=321)
        rej, fold, walk, _ = _both(ctx, feat, hs, None, hs, qs2, full, order, m=321, what="after a 3 kb sequence")
        assert rej[0] + rej[1] * 321 <= qs2.size * 321


def _kmer_bins(codes, k):
    c = codes.astype(np.int64)
    b = np.zeros(c.size - k + 1, dtype=np.int64)
    for i in range(k):
        b = b * 4 + c[i:c.size - k + 1 + i]
    return np.unique(b)


@pytest.mark.gpu
def test_a_set_built_to_collide(ctx):
    """test_a_set_built_to_collide of tests/test_gpu_fold_screen.py: each sequence two copies of its template that differ at every 9th base, so that a related
    pair's OR-folded shared count lies far below the true one -- the slots' own collisions x carry the bound, in the cut as in the screen"""
    n, nq, half = 320, 130, 500
    codes = []
    for t in range(n // FAM):
        tmpl = synth.template(911, t, half)
        second = tmpl.copy()
        second[4::9] = (second[4::9] + 1) & 3
        both = np.concatenate([tmpl, second])
        codes += [synth.member(911, t, j, both, sub_rate=0.005, indel_rate=0.002) for j in range(FAM)]
    seqs = [synth.to_ascii(c) for c in codes]
    hs = api.HistogramSet(ctx, K, 32, n)
    hs.build(seqs)
    text = _text()
    feat = api.Feature.from_text(ctx, text, 0)
    qs = np.arange(nq, dtype=np.uint32)
    rel = (np.arange(n)[None, :] // FAM) == (qs[:, None] // FAM)
    base = _fp64(ctx, feat, hs, None, hs, qs, m=n)
    _both(ctx, feat, hs, None, hs, qs, base, m=n, what="collide, as trained")
    sums = base["sum"]
    for what, by in (("related median", np.median(sums[rel])), ("beside the bulk", float(sums[~rel].max()) + 0.25)):
        moved = _moved(ctx, text, by)
        full = _fp64(ctx, moved, hs, None, hs, qs, m=n)
        _both(ctx, moved, hs, None, hs, qs, full, m=n, what="collide, " + what)


@pytest.mark.gpu
def test_repeat_bearing_queries(ctx, seqs):
    """a 400-base homopolymer in place of 400 bases of every 40th sequence (test_repeat_bearing_queries of tests/test_gpu_fold_screen.py): large bins on both
    sides -- G and the queries' largest excess count in the certificate, P2' in the compare"""
    rep = []
    for i, s in enumerate(seqs):
        s = bytes(s)
        if i % 40 == 1:
            at = 100 + 13 * (i % 40)
            s = s[:at] + b"A" * 400 + s[at + 400:]
        rep.append(s)
    hs = api.HistogramSet(ctx, K, 32, len(rep))
    hs.build(rep)
    qs = np.arange(130, dtype=np.uint32)
    for order in ORDERS:
        feat = api.Feature.from_text(ctx, _text(), 0)
        full = _fp64(ctx, feat, hs, None, hs, qs, order, m=len(rep))
        _both(ctx, feat, hs, None, hs, qs, full, order, m=len(rep), what="repeats")


@pytest.fixture(scope="module")
def flat(seqs):
    """a context made under MSC_TAIL_NO_RAMP (read when a context is made: a call's final tail groups do not halve down to one block), and the set on it"""
    old = os.environ.get("MSC_TAIL_NO_RAMP")
    os.environ["MSC_TAIL_NO_RAMP"] = "1"
    try:
        c = api.Context(0)
    finally:
        if old is None:
            del os.environ["MSC_TAIL_NO_RAMP"]
        else:
            os.environ["MSC_TAIL_NO_RAMP"] = old
    hs = api.HistogramSet(c, K, 32, N)
    hs.build(seqs)
    yield c, hs
    c.close()


@pytest.mark.gpu
def test_tail_groups(flat):
    """3 x 128 queries in ONE tail group, the cut on and off: flags, counts and counters equal, and those of the blocks run one by one"""
    ctx, hs = flat
    feat = api.Feature.from_text(ctx, _text(), 0)
    qs = np.arange(384, dtype=np.uint32)
    full = _fp64(ctx, feat, hs, None, hs, qs, m=N)
    got, rej, fold, walk = _flags(ctx, feat, hs, None, hs, qs, m=N)
    groups = ctx.last_tail_groups()
    _same(got, full)
    off, rej_off, fold_off, walk_off = _flags(ctx, feat, hs, None, hs, qs, m=N, reject=False)
    assert groups == (1, 3) and ctx.last_tail_groups() == (1, 3)
    _same(off, full)
    assert rej_off == (0, 0) and fold == fold_off == (16, 3, 0) and rej[0] > 0 and 0 < walk[0] <= walk_off[0]
    ctx.set_tail_groups(0)
    try:
        rej1, fold1, walk1, _ = _both(ctx, feat, hs, None, hs, qs, full, m=N, what="block by block")
        assert ctx.last_tail_groups() == (0, 0)
    finally:
        ctx.set_tail_groups(8)
    print("tail groups %r: reject %r / block by block %r" % (groups, rej, rej1))
    assert rej == rej1 and fold == fold1 and walk == walk1
