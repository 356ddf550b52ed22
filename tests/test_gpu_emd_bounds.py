"""msc_score_multi's close flags without the dense rank walk (msc_set_emd_bounds, default on; csrc/msc_emd_list.hip): the flags are decided
from exact integer bounds of the earth mover's distance, L = |rk_sum_a - rk_sum_b| <= emd <= rk_dev_a + rk_dev_b = U, and the rank lists
are walked only for the pairs the bounds leave open -- a device list of at most 1/64 of a block's pairs; a block whose list overflows is
scored by the dense walk, on the device. Whatever path a block takes, its flags must be those of the FP64 evaluation of every pair:
"FP64 flags" below is the same call with want=("sum", "close"), which walks every pair's ranks and evaluates every pair in FP64.
msc_last_emd_walk says which path ran.

The 8-bit case runs the model of weights_k9_u32.txt with its Datatype line rewritten (as tests/test_gpu_qxm_direct.py does for other bin
types) and the range of similarity_ratio set to what the statistic takes without the reference's 32-bit wrap (the trained range is that
of the wrapped values, 6.1e-5 .. 6.2e-5; on 8-bit bins the statistic is 0.9997 .. 1 for 1 kb sequences): weights_k9_u8.txt holds no
earth_movers_distance, so a call with it never reaches this path -- asserted below as blocks == 0."""
import numpy as np
import pytest

from golden_util import weights_text
from meshclust2_amd import api, synth

SEED, N, LEN, K, NQ = 20260002, 800, 1000, 9, 130
EMD = 1 << 18
ORDERS = (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST)


def _text(dtype):
    text = weights_text("weights_k9_u32.txt").replace("uint32_t", "uint%d_t" % dtype)
    wrapped = "268435456 6.13962398729182e-05 6.19221396338429e-05"
    assert text.count(wrapped) == 1
    return text if dtype == 32 else text.replace(wrapped, "268435456 0.9997 1")


def _shifted(text, w0):
    """the classification block of a weights file with its intercept replaced (the line after the first `n_combos:`)"""
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("n_combos:")) + 1
    lines[at] = repr(float(w0))
    return "\n".join(lines) + "\n"


def _w0(text):
    lines = text.splitlines()
    return float(lines[next(i for i, ln in enumerate(lines) if ln.startswith("n_combos:")) + 1])


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seqs():
    return synth.families(SEED, N, LEN)[0]


@pytest.fixture(scope="module")
def worlds(ctx, seqs):
    """per bin type: the set, the model and the FP64 evaluation of the 130 x 800 block pair in both argument orders, computed once"""
    out = {}

    def world(dtype):
        if dtype not in out:
            hs = api.HistogramSet(ctx, K, dtype, N)
            for off in range(0, N, 256):
                hs.build(seqs[off:off + 256], first_slot=off)
            text = _text(dtype)
            feat = api.Feature.from_text(ctx, text, 0)
            qs = np.arange(NQ, dtype=np.uint32)
            full = {o: api.score_multi(ctx, feat, hs, None, hs, qs, order=o, m=N, want=("sum", "close", "counts")) for o in ORDERS}
            for o in ORDERS:
                assert np.array_equal(full[o]["close"], (full[o]["sum"] >= 0).astype(np.uint8))
            out[dtype] = dict(hs=hs, text=text, feat=feat, qs=qs, full=full)
        return out[dtype]
    return world


def _flags(ctx, feat, hs, cands, qset, qs, order=api.ORDER_CAND_FIRST, m=None):
    """the close-flag-only call and what msc_last_emd_walk says of it -> (result, listed_pairs, dense_blocks, blocks)"""
    got = api.score_multi(ctx, feat, hs, cands, qset, qs, order=order, m=m, want=("close", "counts"))
    return (got,) + ctx.last_emd_walk()


def _fp64(ctx, feat, hs, cands, qset, qs, order=api.ORDER_CAND_FIRST, m=None):
    full = api.score_multi(ctx, feat, hs, cands, qset, qs, order=order, m=m, want=("sum", "close", "counts"))
    assert np.array_equal(full["close"], (full["sum"] >= 0).astype(np.uint8))
    return full


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [32, 8])
def test_common_path_both_mirror_forms(ctx, seqs, worlds, dtype):
    """130 queries = two blocks (128 rows and 2 rows), both argument orders: flags and counts are the FP64 flags, the flags of the
    switch-off call and (two rows) the oracle's; no block took the dense walk and the listed pairs are within the list's capacity, which
    proves that the list path produced them. Share of pairs listed for this input and model, as this test printed it on an MI355X:
    32-bit bins 961 of 104 000 pairs = 0.92 % in either order, against the capacity of 1.56 % (on the CPU beforehand, 22 of these query
    rows, the weighted sum evaluated in float64 at both ends and the middle of [L, U]: 18 of 17 600 pairs = 0.10 % change sign inside the
    interval -- the screen's product bounds are wider than that, as they must be). 8-bit bins, with the model of this file's head:
    206 of 104 000 pairs = 0.20 %."""
    from oracle import oracle_py
    w = worlds(dtype)
    hs, feat, qs = w["hs"], w["feat"], w["qs"]
    for order in ORDERS:
        full = w["full"][order]
        only, listed, dense, blocks = _flags(ctx, feat, hs, None, hs, qs, order, m=N)
        print("dtype %d order %d: listed %d of %d pairs (%.4f), dense blocks %d of %d" % (dtype, order, listed, NQ * N, listed / (NQ * N), dense, blocks))
        assert ctx.last_kernel_info()[0].startswith("k_pair_gemm_fp4_dma"), ctx.last_kernel_info()
        assert np.array_equal(only["close"], full["close"]) and np.array_equal(only["counts"], full["counts"]), (dtype, order)
        assert blocks == 2 and dense == 0 and 0 < listed <= NQ * N // 64, (listed, dense, blocks)
        ctx.set_emd_bounds(False)
        try:
            off, l0, d0, b0 = _flags(ctx, feat, hs, None, hs, qs, order, m=N)
        finally:
            ctx.set_emd_bounds(True)
        assert np.array_equal(off["close"], only["close"]) and (l0, d0, b0) == (0, 2, 2)
    pred = oracle_py.predictor(w["text"])
    oh = [oracle_py.hist(s, K, dtype) for s in seqs]
    only = _flags(ctx, feat, hs, None, hs, qs, m=N)[0]
    for row in (3, 129):          # (candidate, query) per pair
        f = np.array([oracle_py.score(pred.cls, oh[c], oh[int(qs[row])])[2] >= 0 for c in range(N)], dtype=np.uint8)
        assert np.array_equal(only["close"][row], f), row
    for h in oh:
        oracle_py.lib().orc_hist_free(h)


@pytest.mark.gpu
def test_a_model_without_the_distance_never_reaches_the_path(ctx, seqs):
    """weights_k9_u8.txt (manhattan, pearson, length difference, euclidean): no rank walk to save, no block counted, the same flags"""
    hs = api.HistogramSet(ctx, K, 8, 300)
    hs.build(seqs[:300])
    feat = api.Feature.from_text(ctx, weights_text("weights_k9_u8.txt"), 0)
    qs = np.arange(NQ, dtype=np.uint32)
    full = _fp64(ctx, feat, hs, None, hs, qs, m=300)
    only, listed, dense, blocks = _flags(ctx, feat, hs, None, hs, qs, m=300)
    assert np.array_equal(only["close"], full["close"]) and (listed, dense, blocks) == (0, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [32, 8])
def test_threshold_through_the_listed_pairs(ctx, worlds, dtype):
    """the intercept moved by the median FP64 sum of the same-family pairs: the threshold runs through the pairs the bounds leave open, and
    the exact distances of k_emd_ranks_list decide their flags"""
    w = worlds(dtype)
    hs, qs = w["hs"], w["qs"]
    sums = w["full"][api.ORDER_CAND_FIRST]["sum"]
    same = (np.arange(N)[None, :] // 20) == (qs[:, None] // 20)
    moved = api.Feature.from_text(ctx, _shifted(w["text"], _w0(w["text"]) - float(np.median(sums[same]))), 0)
    full = _fp64(ctx, moved, hs, None, hs, qs, m=N)
    only, listed, dense, blocks = _flags(ctx, moved, hs, None, hs, qs, m=N)
    print("dtype %d: listed %d, dense blocks %d of %d, close among same-family pairs %.3f" % (dtype, listed, dense, blocks, float(full["close"][same].mean())))
    assert 0.3 < float(full["close"][same].mean()) < 0.7          # the boundary really runs through them
    assert np.array_equal(only["close"], full["close"]) and np.array_equal(only["counts"], full["counts"])
    assert listed > 0


@pytest.mark.gpu
def test_overflow_falls_back_on_the_device_and_the_model_remembers(ctx, worlds):
    """the intercept moved by the median sum of ALL pairs: half the pairs sit at the boundary, every block's list overflows and the dense
    walk, queued behind it, produces the flags; a second call with the same model skips the bound pass"""
    w = worlds(32)
    hs, qs = w["hs"], w["qs"]
    sums = w["full"][api.ORDER_CAND_FIRST]["sum"]
    moved = api.Feature.from_text(ctx, _shifted(w["text"], _w0(w["text"]) - float(np.median(sums))), 0)
    full = _fp64(ctx, moved, hs, None, hs, qs, m=N)
    assert 0.45 < float(full["close"].mean()) < 0.55
    first, listed, dense, blocks = _flags(ctx, moved, hs, None, hs, qs, m=N)
    print("first call: listed %d, dense blocks %d of %d" % (listed, dense, blocks))
    assert np.array_equal(first["close"], full["close"]) and np.array_equal(first["counts"], full["counts"])
    assert blocks == 2 and dense == blocks
    again, listed, dense, blocks = _flags(ctx, moved, hs, None, hs, qs, m=N)
    assert np.array_equal(again["close"], full["close"])
    assert listed == 0 and dense == blocks == 2


@pytest.mark.gpu
def test_thirty_two_bit_ranks(ctx, seqs):
    """a 400-base homopolymer spliced into some sequences IN PLACE of 400 of their bases: 400 k-mers in bin 0 put ranks 1 .. 392 at
    -t 4^k / 1024 from the even spread, down to -100 000, which does not fit the 16-bit form (+-32 768), so the set keeps the 32-bit
    mirror only and the listed pairs are walked with v_sad_u32. In place, because the bounds are only as tight as the lists are close to
    the pitch: an inserted run makes the longest list 1 400 and the pitch 1 536, every ordinary row then strays 4^k / 6 per rank from
    base_t, U spans the whole range of the statistic and every block overflows (measured so: listed 0, dense blocks 2 of 2 -- the flags
    were the FP64 flags there too)."""
    rep = []
    for i, s in enumerate(seqs):
        s = bytes(s)
        if i % 9 == 1:
            at = 100 + 13 * (i % 40)
            s = s[:at] + b"A" * 400 + s[at + 400:]
        rep.append(s)
    hs = api.HistogramSet(ctx, K, 32, len(rep))
    hs.build(rep)
    feat = api.Feature.from_text(ctx, _text(32), 0)
    qs = np.arange(NQ, dtype=np.uint32)
    for order in ORDERS:
        full = _fp64(ctx, feat, hs, None, hs, qs, order, m=len(rep))
        only, listed, dense, blocks = _flags(ctx, feat, hs, None, hs, qs, order, m=len(rep))
        print("order %d: listed %d, dense blocks %d of %d" % (order, listed, dense, blocks))
        assert np.array_equal(only["close"], full["close"]) and np.array_equal(only["counts"], full["counts"]), order
        assert listed > 0 and blocks == 2


@pytest.mark.gpu
def test_edges(ctx, seqs, worlds):
    w = worlds(32)
    hs = w["hs"]
    feat = api.Feature.from_text(ctx, w["text"], 0)          # (models of its own: a call whose small list overflows is remembered on the model)
    # an explicit list of 37 slots (with a repeat, out of order), 2 queries
    cands = np.concatenate([np.arange(40, 4, -1, dtype=np.uint32), [7]]).astype(np.uint32)
    assert cands.size == 37
    qs2 = np.array([21, 5], dtype=np.uint32)
    full = _fp64(ctx, feat, hs, cands, hs, qs2)
    only, listed, dense, blocks = _flags(ctx, feat, hs, cands, hs, qs2)
    assert np.array_equal(only["close"], full["close"]) and np.array_equal(only["counts"], full["counts"]) and blocks == 1
    # m = 1: two pairs, a list of no entries -- today's path
    for c in (21, 22, 500):
        one = np.array([c], dtype=np.uint32)
        full = _fp64(ctx, feat, hs, one, hs, qs2)
        only = _flags(ctx, feat, hs, one, hs, qs2)[0]
        assert np.array_equal(only["close"], full["close"]), c
    # queries from a set of another pitch (one 3 kb sequence): today's path, unchanged
    long_seq = synth.families(77, 1, 3000)[0]
    qset = api.HistogramSet(ctx, K, 32, 1)
    qset.build(long_seq)
    qq = np.array([0, 0], dtype=np.uint32)
    full = _fp64(ctx, feat, hs, None, qset, qq, m=N)
    only, listed, dense, blocks = _flags(ctx, feat, hs, None, qset, qq, m=N)
    assert np.array_equal(only["close"], full["close"]) and listed == 0 and dense == blocks and blocks >= 1
    # ten slots rebuilt in place with other sequences: the moments are refreshed with the rows
    hs2 = api.HistogramSet(ctx, K, 32, N)
    hs2.build(seqs)
    qs = np.arange(NQ, dtype=np.uint32)
    feat = api.Feature.from_text(ctx, w["text"], 0)
    before = _flags(ctx, feat, hs2, None, hs2, qs, m=N)[0]
    hs2.build(seqs[600:610], first_slot=100)          # (sequences of the same set: no list longer than the pitch the mirror has)
    full = _fp64(ctx, feat, hs2, None, hs2, qs, m=N)
    only, listed, dense, blocks = _flags(ctx, feat, hs2, None, hs2, qs, m=N)
    print("rebuilt in place: listed %d, dense blocks %d of %d" % (listed, dense, blocks))
    assert np.array_equal(only["close"], full["close"]) and np.array_equal(only["counts"], full["counts"])
    assert not np.array_equal(before["close"], only["close"]) and listed > 0 and dense == 0


def test_bounds_of_the_distance_from_two_moments_cpu():
    """the identity the kernels rely on, in numpy from the oracle's histograms: with the ranks mirror's rows (a_1 .. a_n in bin order, then
    4^k up to the pitch) emd = sum_t |a_t - b_t| is the oracle's earth_movers_distance, and L = |sum a - sum b| <= emd <= sum |a - base| +
    sum |b - base| = U with base_t = floor(t 4^k / pitch) -- padding included (the lengths differ)."""
    from oracle import oracle_py
    k, nbins = 9, 4 ** 9
    seqs, _ = synth.families(515, 300, 1000, family=10, length_jitter=150)
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, 300, (200, 2))
    pairs[:5, 1] = pairs[:5, 0] // 10 * 10          # some same-family pairs, one with itself
    pairs[5] = (17, 17)
    hist, rows = {}, {}
    for i in np.unique(pairs):
        hist[int(i)] = oracle_py.hist(seqs[int(i)], k, 8)
    longest = max(int(h.array().astype(np.int64).sum()) - nbins for h in hist.values())
    pitch = max(256, (longest + 255) // 256 * 256)
    base = np.arange(pitch, dtype=np.int64) * nbins // pitch
    for i, h in hist.items():
        excess = h.array().astype(np.int64) - 1
        assert excess.min() >= 0
        r = np.repeat(np.arange(nbins, dtype=np.int64), excess)
        rows[i] = np.concatenate([r, np.full(pitch - r.size, nbins, dtype=np.int64)])
    slack = []
    for a, b in pairs:
        ra, rb = rows[int(a)], rows[int(b)]
        emd = int(np.abs(ra - rb).sum())
        lo, hi = abs(int(ra.sum()) - int(rb.sum())), int(np.abs(ra - base).sum()) + int(np.abs(rb - base).sum())
        assert lo <= emd <= hi, (a, b, lo, emd, hi)
        assert emd == oracle_py.raw_feature(EMD, hist[int(a)], hist[int(b)]), (a, b)
        slack.append((emd - lo, hi - emd))
    assert min(s[1] for s in slack) > 0          # (the upper bound is never tight for these; the lower one is for a pair with itself)
    for h in hist.values():
        oracle_py.lib().orc_hist_free(h)
