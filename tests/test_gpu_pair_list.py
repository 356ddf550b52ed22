"""msc_score_pair_list on the GPU: an explicit list of pairs against the per-pair 1 x M calls (bit for bit), the CPU oracle (1e-9), the
divergence bits of msc_score_multi, the whole-list pair kernel against the chunked one (two child processes: the library reads
MSC_SPARSE_NO_WL once), the fit rule's boundary, the query-by-query fallback, the error statuses and Predictor.score_pairs against msc_search."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import EXACT, FEATS, weights_text, weights_with_mode
from meshclust2_amd import api
from meshclust2_amd._capi import FEAT_DIV, FEAT_FAST, FEAT_SLOW, MscError
from pair_list_check import LIMIT, call_raw, mixed_sequences, pair_lists, random_with_kmers, score_one

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ORDERS = (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST)
FEAT_GROUPS = api.FEAT["rre_k_r"] | api.FEAT["sim_mm"]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


_SETS = {}


def the_set(ctx, k, dtype, layout, which):
    """one set per (k, dtype, layout, which): which = "mixed" (every sequence) or "short" (450-base mutants in place of the 1 kb ones, no 3 kb ones: the longest
    two lists fit a wave's LDS region together). -> (set, sequences, index of the empty sequence, indices of the 60-120-base ones)"""
    key = (k, dtype, layout, which)
    if key not in _SETS:
        seqs, empty, small = mixed_sequences(k, with_long=which == "mixed")
        hs = api.HistogramSet(ctx, k, dtype, len(seqs), sparse_entries=(sum(len(s) for s in seqs) + 64) if layout == "sparse" else 0)
        hs.build(seqs)
        _SETS[key] = (hs, seqs, empty, small)
    return _SETS[key]


_REF = {}


def per_pair_raw(ctx, hs, key, order, mask):
    """msc_pair_features_raw with m = 1 for every (a, b) of the set, once -> [a][b][columns]"""
    key = ("raw", key, order, mask)
    if key not in _REF:
        n = hs.capacity
        _REF[key] = np.array([[api.pair_features_raw(ctx, hs, [a], hs, b, mask, order)[0] for b in range(n)] for a in range(n)])
    return _REF[key]


def per_pair_score(ctx, feat, hs, key, order, wname):
    """msc_score with m = 1 for every (a, b) of the set, once -> its status and outputs, [a][b]. (A pair with the list of a sequence shorter
    than k has no variance on one side: pearson is NaN and the call returns MSC_ERR_NAN with NaN in the row, as the reference throws.)"""
    key = ("score", key, order, wname)
    if key not in _REF:
        n = hs.capacity
        rows = [[score_one(ctx, feat, hs, a, hs, b, order) for b in range(n)] for a in range(n)]
        ref = {f: np.array([[rows[a][b][i] for b in range(n)] for a in range(n)]) for i, f in enumerate(("rc", "singles", "combos", "sum", "csum"))}
        assert np.isin(ref["rc"], (0, -7)).all() and (ref["rc"] == 0).sum() > n
        assert np.array_equal(np.isnan(ref["sum"]), ref["rc"] != 0)
        _REF[key] = ref
    return _REF[key]


def kernel(ctx):
    name, per_read = ctx.last_kernel_info()
    assert per_read == 1
    return name


CONFIGS = [(8, 16, "dense", "short", "k_pair_sparse_wl_pairs"), (8, 16, "sparse", "short", "k_pair_sparse_wl_pairs"),
           (8, 16, "dense", "mixed", "k_pair_sparse_mp"), (8, 16, "sparse", "mixed", "k_pair_sparse_mp"),
           (5, 16, "dense", "mixed", "k_pair_tiles_batch"), (11, 32, "sparse", "short", "k_pair_sparse_wl_pairs"), (11, 32, "sparse", "mixed", "k_pair_sparse_mp")]


@pytest.mark.parametrize("k,dtype,layout,which,expect", CONFIGS, ids=["k%d_u%d_%s_%s" % c[:4] for c in CONFIGS])
def test_rows_equal_the_per_pair_calls(ctx, k, dtype, layout, which, expect):
    """1. raw_out (FEAT_FAST, both orders: the u32 simratio wrap on both sides) == msc_pair_features_raw per pair, singles / combos / sum /
    csum / close == msc_score per pair (k = 8: weights_k8_u16.txt), array_equal, on every pair list; the kernel each call names."""
    hs, seqs, empty, small = the_set(ctx, k, dtype, layout, which)
    key = (k, dtype, layout, which)
    feat = api.Feature.from_text(ctx, weights_text("weights_k8_u16.txt"), 0) if k == 8 else None
    lists = pair_lists(len(seqs), empty, small)
    for order in ORDERS:
        ref = per_pair_raw(ctx, hs, key, order, FEAT_FAST)
        sc = per_pair_score(ctx, feat, hs, key, order, "k8") if feat is not None else None
        for name, (a, b) in lists.items():
            got = api.score_pair_list(ctx, None, hs, a, hs, b, order, FEAT_FAST)
            assert kernel(ctx).startswith(expect), (name, kernel(ctx))
            assert got["raw"].shape == (len(a), 9) and got["sum"] is None
            assert np.array_equal(got["raw"], ref[a, b], equal_nan=True), (name, order)
            if feat is None or (name == "many" and order != ORDERS[0]):
                continue
            rc, got = call_raw(ctx, feat, hs, a, hs, b, order, 0)
            assert rc == sc["rc"][a, b].min(), (name, order, rc)          # the status of the per-pair calls: MSC_OK, or MSC_ERR_NAN where a row has it
            assert kernel(ctx).startswith(expect), (name, kernel(ctx))
            for f in ("singles", "combos", "sum", "csum"):
                assert np.array_equal(got[f], sc[f][a, b], equal_nan=True), (name, order, f)
            with np.errstate(invalid="ignore"):
                assert np.array_equal(got["close"], (np.round(sc["csum"][a, b]) > 0).astype(np.uint8)), (name, order)
            if rc == 0:          # the api's own wrappers (they raise on a status)
                s2, c2 = feat.compute_pairs(hs, a, hs, b, order)
                d2 = api.score_pair_list(ctx, feat, hs, a, hs, b, order, FEAT_FAST)
                assert np.array_equal(s2, got["singles"]) and np.array_equal(c2, got["combos"]), name
                assert np.array_equal(d2["sum"], got["sum"]) and np.array_equal(d2["close"], got["close"]) and np.array_equal(d2["raw"], ref[a, b], equal_nan=True), name
    # NULL slot lists mean slots 0 .. n-1
    n = len(seqs)
    ident = np.arange(n, dtype=np.uint32)
    got = api.score_pair_list(ctx, None, hs, None, hs, None, ORDERS[0], FEAT_FAST, n=n)
    assert np.array_equal(got["raw"], per_pair_raw(ctx, hs, key, ORDERS[0], FEAT_FAST)[ident, ident], equal_nan=True)
    got = api.score_pair_list(ctx, None, hs, ident[::-1].copy(), hs, None, ORDERS[0], FEAT_FAST)
    assert np.array_equal(got["raw"], per_pair_raw(ctx, hs, key, ORDERS[0], FEAT_FAST)[ident[::-1], ident], equal_nan=True)


ORACLE_CONFIGS = [(5, 16, "dense", "weights_k5_u16_slow.txt", " per query"), (6, 16, "dense", "weights_mixed_slow_k6_u16.txt", " per query"),
                  (8, 16, "dense", None, "k_pair_sparse_mp"), (8, 16, "sparse", None, "k_pair_sparse_mp")]


@pytest.mark.parametrize("k,dtype,layout,wname,expect", ORACLE_CONFIGS, ids=["k%d_%s" % (c[0], c[2]) for c in ORACLE_CONFIGS])
def test_rows_against_the_cpu_oracle(ctx, oracle, k, dtype, layout, wname, expect):
    """2. every statistic of FEAT_SLOW against oracle.raw_feature and the weighted sums of the --feat slow fixtures against oracle.score: integer
    statistics equal, FP64 ones to 1e-9 relative (the standing tolerance of tests/test_gpu_parity.py). The divergence statistics of histograms
    under 64 KiB come query by query; from 64 KiB on, from the pair-list form of the chunked merge kernel."""
    hs, seqs, empty, small = the_set(ctx, k, dtype, layout, "mixed")
    oh = [oracle.hist(s, k, dtype) for s in seqs]
    lists = pair_lists(len(seqs), empty, small)
    lists.pop("many")
    lists["random"] = (lists["random"][0][40:140].copy(), lists["random"][1][40:140].copy())          # (the oracle walks 4^k bins per statistic)
    for order in ORDERS:
        for name, (a, b) in lists.items():
            got = api.score_pair_list(ctx, None, hs, a, hs, b, order, FEAT_SLOW)["raw"]
            assert kernel(ctx).startswith(expect) if expect[0] != " " else kernel(ctx).endswith(expect), (name, kernel(ctx))
            for i in range(len(a)):
                x, y = (oh[a[i]], oh[b[i]]) if order == api.ORDER_CAND_FIRST else (oh[b[i]], oh[a[i]])
                for col, (fname, bit) in enumerate(FEATS):
                    exp = oracle.raw_feature(1 << bit, x, y)
                    if np.isnan(exp):
                        assert np.isnan(got[i][col]), (name, order, i, fname)
                    elif fname in EXACT:
                        assert got[i][col] == exp, (name, order, i, fname)
                    else:
                        assert got[i][col] == pytest.approx(exp, rel=1e-9, abs=1e-13), (name, order, i, fname)
    if wname is None:
        return
    text = weights_text(wname)
    feat = api.Feature.from_text(ctx, text, 0)
    pred = oracle.predictor(text)
    a, b = lists["random"]
    keep = (a >= 3) & (b >= 3)          # (a sequence of k + 1 bases and less leaves pearson without a variance: the reference throws there)
    a, b = a[keep].copy(), b[keep].copy()
    got = api.score_pair_list(ctx, feat, hs, a, hs, b, api.ORDER_CAND_FIRST, 0, want=("sum", "singles", "combos"))
    # (the statistics a selection kept decide: a --feat slow model without a divergence statistic takes the dense pair-list kernel)
    has_div = any(f & FEAT_DIV for f in feat.single_flags())
    assert kernel(ctx).endswith(" per query") if has_div else kernel(ctx).startswith("k_pair_tiles_batch"), kernel(ctx)
    for i in range(len(a)):
        s, c, w = oracle.score(pred.cls, oh[a[i]], oh[b[i]])
        assert np.allclose(got["singles"][i], s, rtol=1e-9, atol=1e-12) and np.allclose(got["combos"][i], c, rtol=1e-9, atol=1e-12), i
        assert got["sum"][i] == pytest.approx(w, rel=1e-9, abs=1e-12), i


@pytest.mark.parametrize("layout", ["dense", "sparse"])
def test_divergence_bits_are_those_of_score_multi(ctx, layout):
    """3. feat_mask = MSC_FEAT_DIV at k = 8 / u16: the pair list's two sums are msc_score_multi's raw_out entries of the same (query, candidate)
    bit for bit, and the same list reordered and cut into two calls gives the same bits per pair."""
    hs, seqs, empty, small = the_set(ctx, 8, 16, layout, "mixed")
    n = len(seqs)
    everyone = np.arange(n, dtype=np.uint32)
    lists = pair_lists(n, empty, small)
    for order in ORDERS:
        multi = api.score_multi(ctx, None, hs, everyone, hs, everyone, order, feat_mask=FEAT_DIV)["raw"]          # [query][candidate][2]
        for name in ("self", "with_empty", "random", "one", "five"):
            a, b = lists[name]
            got = api.score_pair_list(ctx, None, hs, a, hs, b, order, FEAT_DIV)["raw"]
            assert kernel(ctx).startswith("k_pair_sparse_mp"), kernel(ctx)
            assert np.array_equal(got, multi[b, a]), (name, order)
        a, b = lists["random"]
        perm = np.random.default_rng(5).permutation(len(a))
        cut = len(a) // 3
        whole = api.score_pair_list(ctx, None, hs, a, hs, b, order, FEAT_DIV)["raw"]
        for part in (perm[:cut], perm[cut:]):
            got = api.score_pair_list(ctx, None, hs, a[part], hs, b[part], order, FEAT_DIV)["raw"]
            assert np.array_equal(got, whole[part]), order


_TROUBLE = []          # a child that faulted, aborted or hung: nothing more is started on the GPU after one


def run_child(out_dir, switches, expect, timeout=120):
    if _TROUBLE:
        pytest.fail("not started: an earlier child ended with %s" % _TROUBLE[0])
    env = dict(os.environ)
    env.pop("MSC_SPARSE_NO_WL", None)
    for sw in switches.split():
        env[sw] = "1"
    env["MSC_TEST_EXPECT_KERNEL"] = expect
    try:
        out = subprocess.run([sys.executable, os.path.join(HERE, "pair_list_check.py"), str(out_dir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired:
        _TROUBLE.append("no result within %d s" % timeout)
        raise
    if out.returncode not in (0, 1):          # (1: a failed check; anything else -- an abort, a signal -- may have left the GPU in trouble)
        _TROUBLE.append("exit status %d" % out.returncode)
    assert b"PAIR_LIST_OK" in out.stdout, out.stdout.decode(errors="replace")[-3000:]


def test_whole_list_kernel_against_the_chunked_one(tmp_path):
    """4. child A (defaults) reports k_pair_sparse_wl_pairs on the short-list sets, child B (MSC_SPARSE_NO_WL) k_pair_sparse_mp; their
    non-divergence statistics are array_equal."""
    run_child(tmp_path / "a", "", "k_pair_sparse_wl_pairs")
    run_child(tmp_path / "b", "MSC_SPARSE_NO_WL", "k_pair_sparse_mp")
    names = sorted(p.name for p in (tmp_path / "a").iterdir() if p.suffix == ".npy")
    assert len(names) >= 8, names
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.shape == y.shape and x.size and np.array_equal(x, y, equal_nan=True), f


def test_fit_boundary(ctx):
    """5. two sparse sets whose longest lists sum to exactly the rule's limit take the whole-list kernel, one entry more the chunked one; both
    equal the per-pair calls."""
    k, dtype = 11, 32
    half = LIMIT // 2

    def build(entries, seed):
        seqs = [random_with_kmers(seed, k, entries), random_with_kmers(seed + 1, k, 40), b"ACG"]
        hs = api.HistogramSet(ctx, k, dtype, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 64)
        hs.build(seqs)
        assert hs.build_info()[3] == entries, hs.build_info()
        return hs
    a_set = build(half, 100)
    for b_entries, expect in ((LIMIT - half, "k_pair_sparse_wl_pairs"), (LIMIT - half + 1, "k_pair_sparse_mp")):
        b_set = build(b_entries, 200)
        assert a_set.build_info()[3] + b_set.build_info()[3] == LIMIT + (expect == "k_pair_sparse_mp")
        a = np.repeat(np.arange(3, dtype=np.uint32), 3)
        b = np.tile(np.arange(3, dtype=np.uint32), 3)
        for order in ORDERS:
            got = api.score_pair_list(ctx, None, a_set, a, b_set, b, order, FEAT_FAST)["raw"]
            assert kernel(ctx).startswith(expect), kernel(ctx)
            ref = np.array([api.pair_features_raw(ctx, a_set, [a[i]], b_set, int(b[i]), FEAT_FAST, order)[0] for i in range(len(a))])
            assert np.array_equal(got, ref, equal_nan=True), (expect, order)


def test_fallback_and_errors(ctx):
    """6. MSC_FEAT_GROUPS goes query by query (the name ends in " per query") with the per-pair values; a slot of length 0 gives
    MSC_ERR_ZERO_LENGTH with NaN in its rows only; an out-of-range slot, unequal k and -- like every 1 x M call, whose validate_pair the
    fallback would meet -- one dense with one sparse set are MSC_ERR_INVALID_ARG."""
    hs, seqs, empty, small = the_set(ctx, 8, 16, "dense", "short")
    sp = the_set(ctx, 8, 16, "sparse", "short")[0]
    n = len(seqs)
    a, b = pair_lists(n, empty, small)["random"]
    mask = FEAT_FAST | FEAT_GROUPS
    for s in (hs, sp):
        got = api.score_pair_list(ctx, None, s, a, s, b, ORDERS[0], mask)["raw"]
        assert kernel(ctx).endswith(" per query"), kernel(ctx)
        ref = np.array([api.pair_features_raw(ctx, s, [a[i]], s, int(b[i]), mask, ORDERS[0])[0] for i in range(len(a))])
        assert np.array_equal(got, ref, equal_nan=True)
    # one dense and one sparse set: refused by the 1 x M calls, so by this one
    with pytest.raises(MscError) as e:
        api.pair_features_raw(ctx, hs, [1], sp, 2, FEAT_FAST)
    assert e.value.code == -1
    rc, _ = call_raw(ctx, None, hs, a, sp, b, ORDERS[0], FEAT_FAST)
    assert rc == -1
    # a slot of length 0
    k5, s5, e5, sm5 = the_set(ctx, 5, 16, "dense", "mixed")
    z = api.HistogramSet(ctx, 5, 16, 4)
    z.build(s5[3:6], first_slot=0)
    z.upload(3, np.ones(4 ** 5, dtype=np.uint16), 0)
    a = np.array([0, 3, 1, 2, 3, 0], dtype=np.uint32)
    b = np.array([1, 0, 3, 2, 3, 0], dtype=np.uint32)
    bad = (a == 3) | (b == 3)
    feat = api.Feature.from_text(ctx, weights_text("weights_k5_u16.txt"), 0)
    for order in ORDERS:
        rc, got = call_raw(ctx, feat, z, a, z, b, order, FEAT_FAST)
        assert rc == -6, rc
        assert kernel(ctx).startswith("k_pair_tiles_batch")
        for i in range(len(a)):
            ref = np.zeros((1, 9))
            s_ref, cs_ref = np.zeros(1), np.zeros(1)
            sl = np.array([a[i]], dtype=np.uint32)
            rc1 = ctx.lib.msc_pair_features_raw(ctx.h, z.h, sl.ctypes.data_as(C.c_void_p), 1, z.h, int(b[i]), order, FEAT_FAST, ref.ctypes.data_as(C.c_void_p))
            rc2 = ctx.lib.msc_score(ctx.h, feat.h, z.h, sl.ctypes.data_as(C.c_void_p), 1, z.h, int(b[i]), order, None, None, s_ref.ctypes.data_as(C.c_void_p),
                                    cs_ref.ctypes.data_as(C.c_void_p))
            assert (rc1, rc2) == ((-6, -6) if bad[i] else (0, 0)), (i, rc1, rc2)
            assert np.array_equal(got["raw"][i], ref[0], equal_nan=True), i
            assert np.array_equal(got["sum"][i:i + 1], s_ref, equal_nan=True) and np.array_equal(got["csum"][i:i + 1], cs_ref, equal_nan=True), i
            assert np.isnan(got["raw"][i]).any() == bad[i] and np.isnan(got["sum"][i]) == bad[i], i
            assert got["close"][i] == (0 if bad[i] else int(np.round(cs_ref[0]) > 0)), i
    # argument checks
    rc, _ = call_raw(ctx, None, z, np.array([0, 4], dtype=np.uint32), z, np.array([0, 1], dtype=np.uint32), ORDERS[0], FEAT_FAST)
    assert rc == -1
    rc, _ = call_raw(ctx, None, z, np.array([0, 1], dtype=np.uint32), z, np.array([0, 9], dtype=np.uint32), ORDERS[0], FEAT_FAST)
    assert rc == -1
    rc, _ = call_raw(ctx, None, z, np.array([0], dtype=np.uint32), hs, np.array([0], dtype=np.uint32), ORDERS[0], FEAT_FAST)          # k = 5 against k = 8
    assert rc == -1
    rc, _ = call_raw(ctx, feat, hs, np.array([0], dtype=np.uint32), hs, np.array([0], dtype=np.uint32), ORDERS[0], 0)          # a k = 5 model on k = 8 sets
    assert rc == -1
    assert ctx.lib.msc_score_pair_list(ctx.h, None, z.h, None, z.h, None, 2, 0, FEAT_FAST, None, None, None, None, None, None) == -1          # no output at all
    assert ctx.lib.msc_score_pair_list(ctx.h, None, z.h, None, z.h, None, 0, 0, FEAT_FAST, None, None, None, None, None, None) == 0          # n == 0


@pytest.mark.parametrize("mode", [3, 1, 2])
@pytest.mark.parametrize("layout", ["dense", "sparse"])
def test_predictor_score_pairs_is_msc_search_per_pair(ctx, layout, mode):
    """7. Predictor.score_pairs == msc_search for the same pairs, flags and similarity bits, with a two-block weights text (and its mode 1 /
    mode 2 cuts) at k = 8."""
    text = weights_text("weights_k9_u32_fc.txt").replace("k: 9", "k: 8")
    if mode != 3:
        text = weights_with_mode(text, mode)
    pred = api.Predictor.from_text(ctx, text)
    assert (pred.cls is not None, pred.reg is not None) == (bool(mode & 1), bool(mode & 2))
    hs, seqs, empty, small = the_set(ctx, 8, 16, layout, "short")
    a, b = pair_lists(len(seqs), empty, small)["random"]
    a, b = np.maximum(a, 3), np.maximum(b, 3)          # (pairs of real sequences: msc_search stops at a row the reference would throw for)
    close, sim = pred.score_pairs(hs, a, hs, b)
    for q in np.unique(b):
        idx = np.nonzero(b == q)[0]
        c1, s1 = pred.search(hs, a[idx], hs, int(q))
        assert np.array_equal(close[idx], c1) and np.array_equal(sim[idx], s1), (mode, q)
    assert ((sim >= 0) & (sim <= 1)).all()
    if mode == 2:
        assert close.all()
    if mode == 1:
        assert (sim == 1).all()
