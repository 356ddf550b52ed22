"""Shared inputs of tests/test_gpu_pair_list.py and, run as a script, the checker of its route test: one process = one setting of
MSC_SPARSE_NO_WL (the library reads it once). As a script it scores the pair lists of the short-list sets (two sparse sets, and dense sets
through their mirrors), asserts that every call names the kernel in MSC_TEST_EXPECT_KERNEL, checks a sample of rows against the per-pair
calls, dumps the non-divergence statistics of every list to <out_dir>/*.npy and prints PAIR_LIST_OK. Exit status 1 = a failed check."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)



def _fit_limit():
    """the fit rule of k_pair_sparse_wl_pairs (msc_sparse_wl_pairs_fits): the two sets' longest lists hold at most this many
    entries together -- a wave's LDS entries, read from the one place that states them (kWlPairsEntries in csrc/sparse.hip), less two
    predecessor and two end-marker entries. test_fit_boundary holds the routing the calls report to this number on both sides."""
    import re
    src = open(os.path.join(ROOT, "meshclust2_amd", "csrc", "sparse.hip")).read()
    found = re.findall(r"constexpr\s+uint32_t\s+kWlPairsEntries\s*=\s*(\d+)\s*;", src)
    assert len(found) == 1, found
    return int(found[0]) - 4


LIMIT = _fit_limit()
# the "short" sets below (450-base mutants, under 450 entries a list) are meant to fit the rule whatever it is between these two
assert 1020 <= LIMIT <= 2044, LIMIT


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def random_with_kmers(seed, k, entries):
    """a random sequence trimmed base by base until it holds exactly `entries` distinct k-mers (= stored bins of its sparse slot)"""
    rng = np.random.default_rng(seed)
    s = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, entries + k + 40)])
    while len({s[i:i + k] for i in range(len(s) - k + 1)}) > entries:
        s = s[:-1]
    assert len({s[i:i + k] for i in range(len(s) - k + 1)}) == entries
    return s


def mixed_sequences(k, with_long=True):
    """-> (sequences, index of the one shorter than k (an empty list), indices of the 60-120-base ones). In order: fewer than k bases, k and
    k + 1 bases (one or two entries), eight of 60-120 bases, four mutants of one template (~1 kb with_long, else 450 bases: two such lists fit
    a wave's LDS region together), one with a homopolymer run (values >= 3 and one count past 255), and -- with_long -- two of 3 kb."""
    from meshclust2_amd import synth
    rng = np.random.default_rng(1234 + k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rnd(n):
        return bytes(acgt[rng.integers(0, 4, n)])
    seqs = [rnd(k - 1), rnd(k), rnd(k + 1)]
    small = list(range(len(seqs), len(seqs) + 8))
    seqs += [rnd(int(n)) for n in rng.integers(60, 121, 8)]
    seqs += synth.families(4242 + k, 4, 990 if with_long else 450, family=4)[0]
    seqs.append(rnd(60) + b"A" * 300 + rnd(50) + b"ACACACACAC" * 3 + rnd(40))
    if with_long:
        seqs += synth.families(777 + k, 2, 3000, family=2)[0]
    return seqs, 0, small


def pair_lists(n, empty, small):
    """name -> (a, b) uint32 arrays: every sequence with itself, every sequence with the empty one in both positions, 300 random pairs with
    repeats and shared and distinct b, n = 1, n = 5, and 20 000 pairs over the 60-120-base sequences (more pairs than resident waves)"""
    rng = np.random.default_rng(99)
    u = lambda x: np.ascontiguousarray(x, dtype=np.uint32)          # noqa: E731
    everyone = np.arange(n)
    out = {"self": (u(everyone), u(everyone)),
           "with_empty": (u(np.concatenate([everyone, np.full(n, empty)])), u(np.concatenate([np.full(n, empty), everyone])))}
    a, b = rng.integers(0, n, 300), rng.integers(0, n, 300)
    b[:60] = b[0]                                     # a long run of one b ...
    a[100:120], b[100:120] = a[100], b[100]           # ... and a repeated pair
    out["random"] = (u(a), u(b))
    out["one"] = (u([n - 1]), u([n // 2]))
    out["five"] = (u(a[:5]), u(b[200:205]))
    sm = np.asarray(small)
    out["many"] = (u(sm[rng.integers(0, sm.size, 20000)]), u(sm[rng.integers(0, sm.size, 20000)]))
    return out


def call_raw(ctx, feat, a_set, a, b_set, b, order, feat_mask):
    """msc_score_pair_list without the exception: -> (status, dict of every output the arguments allow)"""
    n = len(a)
    nf = bin(feat_mask).count("1")
    raw = np.zeros((n, nf)) if nf else None
    s = cs = close = singles = combos = None
    if feat is not None:
        s, cs, close = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8)
        singles, combos = np.zeros((n, feat.n_singles)), np.zeros((n, feat.n_combos))
    rc = ctx.lib.msc_score_pair_list(ctx.h, feat.h if feat is not None else None, a_set.h, _ptr(a), b_set.h, _ptr(b), n, order, feat_mask, _ptr(raw), _ptr(singles),
                                     _ptr(combos), _ptr(s), _ptr(cs), _ptr(close))
    return rc, dict(raw=raw, sum=s, csum=cs, close=close, singles=singles, combos=combos)


def score_one(ctx, feat, cands, a, qset, b, order):
    """msc_score for the one pair (a, b) without the exception -> (status, singles, combos, sum, csum)"""
    sl = np.array([a], dtype=np.uint32)
    singles, combos, s, cs = np.zeros(feat.n_singles), np.zeros(feat.n_combos), np.zeros(1), np.zeros(1)
    rc = ctx.lib.msc_score(ctx.h, feat.h, cands.h, _ptr(sl), 1, qset.h, int(b), order, _ptr(singles), _ptr(combos), _ptr(s), _ptr(cs))
    return rc, singles, combos, s[0], cs[0]


def main(out_dir):
    from meshclust2_amd import api
    from meshclust2_amd._capi import FEAT_FAST
    os.makedirs(out_dir, exist_ok=True)
    expect = os.environ["MSC_TEST_EXPECT_KERNEL"]
    ctx = api.Context(0)
    failed = []
    for k, dtype, layout in ((8, 16, "sparse"), (8, 16, "dense"), (9, 32, "sparse")):
        seqs, empty, small = mixed_sequences(k, with_long=False)
        hs = api.HistogramSet(ctx, k, dtype, len(seqs), sparse_entries=(sum(len(s) for s in seqs) + 64) if layout == "sparse" else 0)
        hs.build(seqs)
        for name, (a, b) in pair_lists(len(seqs), empty, small).items():
            for order in (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST):
                raw = api.score_pair_list(ctx, None, hs, a, hs, b, order, FEAT_FAST)["raw"]
                got = ctx.last_kernel_info()[0]
                if not got.startswith(expect):
                    failed.append(("kernel", k, layout, name, got))
                for i in range(0, len(a), max(1, len(a) // 25)):          # a sample of rows against the per-pair call
                    ref = api.pair_features_raw(ctx, hs, [a[i]], hs, int(b[i]), FEAT_FAST, order)[0]
                    if not np.array_equal(raw[i], ref, equal_nan=True):
                        failed.append(("row", k, layout, name, order, i))
                np.save(os.path.join(out_dir, "k%d_%s_%s_%d.npy" % (k, layout, name, order)), raw)
    ctx.close()
    if failed:
        print("FAILED", failed[:10])
        return 1
    print("PAIR_LIST_OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
