"""msc_search_pairs: fastcar's work() (fastcar/FC_Runner.cpp:426-471) for many queries with the close pairs and their similarity as the only
output. Held to the dense Q x M path (msc_score_multi's close flags and regression sums, rebuilt into the same list) bit for bit, to msc_search
per query, and to the reference's own fastcar output -- on the matrix-core route and on the fallback through the older routes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLDEN, weights_text
from meshclust2_amd import api, synth

pytestmark = pytest.mark.gpu
GEMM = "k_pair_gemm_fp4_dma<"


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _set(ctx, seqs, k, dtype, sparse=False, strip=False):
    hs = api.HistogramSet(ctx, k, dtype, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 1024 if sparse else 0)
    for off in range(0, len(seqs), 256):
        hs.build(seqs[off:off + 256], first_slot=off, strip=strip)
    return hs


def _with_mode(text, mode):
    return text.replace("mode: 3", "mode: %d" % mode, 1)


def _dense_list(ctx, pred, db, db_slots, qset, q_slots, m, win_lo=None, win_hi=None):
    """the list rebuilt from the dense path: score_multi's close flags (every pair without a classification block) and its regression sums,
    clamped as p_predict does (1 without a regression block)"""
    nq = len(q_slots)
    close = np.ones((nq, m), dtype=np.uint8)
    sim = np.ones((nq, m))
    if pred.cls is not None:
        close = api.score_multi(ctx, pred.cls, db, db_slots, qset, q_slots, m=m, want=("close",))["close"]
    if pred.reg is not None:
        sim = np.clip(api.score_multi(ctx, pred.reg, db, db_slots, qset, q_slots, m=m, want=("sum",))["sum"], 0.0, 1.0)
    offsets, idx, val = [0], [], []
    for q in range(nq):
        lo, hi = (0, m) if win_lo is None else (int(win_lo[q]), min(int(win_hi[q]), m))
        hit = np.nonzero(close[q, lo:hi])[0] + lo if hi > lo else np.zeros(0, dtype=np.int64)
        idx.append(hit)
        val.append(sim[q, hit])
        offsets.append(offsets[-1] + hit.size)
    return np.array(offsets, dtype=np.uint64), np.concatenate(idx).astype(np.uint32), np.concatenate(val)


def _same(got, exp, where):
    offsets, idx, sim, _ = got
    e_off, e_idx, e_sim = exp
    assert np.array_equal(offsets, e_off), where
    assert np.array_equal(idx, e_idx), where
    assert np.array_equal(sim.view(np.uint64), e_sim.view(np.uint64)), where          # bit for bit


@pytest.fixture(scope="module")
def k9(ctx):
    seqs, _ = synth.families(9090, 300, 1000, family=20)
    return _set(ctx, seqs, 9, 32), len(seqs)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_list_equals_the_dense_path_on_the_matrix_cores(ctx, k9, mode):
    hs, n = k9
    pred = api.Predictor.from_text(ctx, _with_mode(weights_text("weights_k9_u32_fc.txt"), mode))
    q = np.arange(n, dtype=np.uint32)          # 300 queries: blocks of 128, 128, 44
    got = pred.search_pairs(hs, None, hs, q, m=n)
    assert got[3]["route"] == api.PAIRS_ROUTE_MATRIX, got[3]
    assert ctx.last_kernel_info()[0].startswith(GEMM), ctx.last_kernel_info()
    assert got[3]["n_pairs"] == int(got[0][-1]) and got[3]["n_pairs"] > n
    if mode & 2:
        assert got[3]["fp64_pairs"] >= got[3]["n_pairs"]          # the regression evaluations
    _same(got, _dense_list(ctx, pred, hs, None, hs, q, n), mode)
    # a slot list in another order: candidate indices are positions in it
    perm = np.random.default_rng(mode).permutation(n).astype(np.uint32)
    _same(pred.search_pairs(hs, perm, hs, q[:130]), _dense_list(ctx, pred, hs, perm, hs, q[:130], n), (mode, "perm"))


def test_windows_bound_the_list(ctx, k9):
    hs, n = k9
    pred = api.Predictor.from_text(ctx, weights_text("weights_k9_u32_fc.txt"))
    rng = np.random.default_rng(7)
    q = np.arange(n, dtype=np.uint32)
    lo = rng.integers(0, n, size=n).astype(np.uint64)
    hi = np.minimum(lo + rng.integers(0, 120, size=n), n + 5).astype(np.uint64)          # (win_hi past m is clamped)
    lo[::17] = hi[::17]                                                               # empty windows
    lo[5::23] = hi[5::23] + 3                                                         # lo > hi: empty too
    got = pred.search_pairs(hs, None, hs, q, win_lo=lo, win_hi=hi, m=n)
    assert got[3]["route"] == api.PAIRS_ROUTE_MATRIX
    offsets, idx = got[0], got[1]
    for j in range(n):
        row = idx[offsets[j]:offsets[j + 1]]
        assert np.all(row >= lo[j]) and np.all(row < hi[j]), j
    _same(got, _dense_list(ctx, pred, hs, None, hs, q, n, np.minimum(lo, hi), hi), "windows")
    # every window empty: nothing listed
    none = pred.search_pairs(hs, None, hs, q, win_lo=hi, win_hi=hi, m=n)
    assert none[3]["n_pairs"] == 0 and not np.any(none[0])


@pytest.mark.parametrize("case", ["k5_u16", "k13_sparse", "cfg5_slow", "one_query"])
def test_fallback_route_gives_the_same_list(ctx, k9, case):
    seqs, _ = synth.families(5150, 300, 1000, family=20)
    if case == "k5_u16":
        hs, text = _set(ctx, seqs, 5, 16), weights_text("weights_k5_u16.txt")
    elif case == "k13_sparse":
        hs, text = _set(ctx, seqs, 13, 64, sparse=True), weights_text("weights_cfg4_k13.txt")
    elif case == "cfg5_slow":
        hs, text = _set(ctx, seqs, 9, 8), weights_text("weights_cfg5_k9.txt")
    else:
        hs, text = k9[0], weights_text("weights_k9_u32_fc.txt")
    n = len(seqs)
    pred = api.Predictor.from_text(ctx, text)
    q = np.arange(1 if case == "one_query" else 140, dtype=np.uint32)
    got = pred.search_pairs(hs, None, hs, q, m=n)
    assert got[3]["route"] == api.PAIRS_ROUTE_FALLBACK, got[3]
    _same(got, _dense_list(ctx, pred, hs, None, hs, q, n), case)
    for j in (0, len(q) // 2, len(q) - 1):          # rows held to msc_search
        close, sim = pred.search(hs, None, hs, int(q[j]), m=n)
        hit = np.nonzero(close)[0]
        a, b = int(got[0][j]), int(got[0][j + 1])
        assert np.array_equal(got[1][a:b], hit), (case, j)
        assert np.array_equal(got[2][a:b].view(np.uint64), sim[hit].view(np.uint64)), (case, j)


def _libstdcxx_sort_order(keys):
    """the permutation libstdc++'s std::sort (introsort, then the final insertion sort) leaves for `keys` under <: fastcar sorts its database
    with it (FC_Runner.cpp:590-592), and equal lengths keep that order in its output"""
    a = list(range(len(keys)))

    def less(x, y):
        return keys[x] < keys[y]

    def median_to_first(res, p, q, r):
        if less(a[p], a[q]):
            t = q if less(a[q], a[r]) else r if less(a[p], a[r]) else p
        elif less(a[p], a[r]):
            t = p
        else:
            t = r if less(a[q], a[r]) else q
        a[res], a[t] = a[t], a[res]

    def partition(first, last, pivot):
        while True:
            while less(a[first], a[pivot]):
                first += 1
            last -= 1
            while less(a[pivot], a[last]):
                last -= 1
            if not first < last:
                return first
            a[first], a[last] = a[last], a[first]
            first += 1

    def loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                raise NotImplementedError("the heap-sort branch of introsort")
            depth -= 1
            median_to_first(first, first + 1, first + (last - first) // 2, last - 1)
            cut = partition(first + 1, last, first)
            loop(cut, last, depth)
            last = cut

    def linear_insert(i):
        v, j = a[i], i - 1
        while less(v, a[j]):
            a[i], i, j = a[j], j, j - 1
        a[i] = v

    def insertion_sort(first, last):
        for i in range(first + 1, last):
            if less(a[i], a[first]):
                a[first:i + 1] = [a[i]] + a[first:i]
            else:
                linear_insert(i)

    n = len(a)
    if n:
        loop(0, n, 2 * (n.bit_length() - 1))
        insertion_sort(0, min(n, 16))
        for i in range(16, n):
            linear_insert(i)
    return a


def test_reference_fastcar_bytes_from_the_new_call(ctx):
    """The inputs of test_gpu_qxm_direct.py's fastcar k = 9 / uint32_t test, searched through search_pairs from Python with fastcar's own
    windows (bin_search, FC_Runner.cpp:389-407,437-444) and printed as fastcar prints: the reference's output byte for byte."""
    db, h = synth.families(43, 220, 1000, family=10, length_jitter=120)
    qs, hq = synth.families(43, 30, 1000, family=10, length_jitter=120)
    runs = [b"A" * 300, b"AC" * 150, b"ACGTTGCAAGTC" * 10]
    db = [s[:200 + i] + runs[(i // 9) % 3] + s[200 + i:] if i % 9 == 4 else s for i, s in enumerate(db)]
    qs = [x[:len(x) - 5] for x in qs]
    qs[4] = qs[4][:333] + runs[0] + qs[4][333:]
    hq = [x.replace(">seq", ">qry") for x in hq]
    dset, qset = _set(ctx, db, 9, 32, strip=True), _set(ctx, qs, 9, 32, strip=True)
    dlen, qlen = [int(x) for x in dset.lengths()], [int(x) for x in qset.lengths()]
    order = _libstdcxx_sort_order(dlen)
    plen = [dlen[i] for i in order]

    def bin_search(begin, last, length):
        if last < begin:
            return 0
        idx = begin + (last - begin) // 2
        if plen[idx] == length:
            while idx > 0 and plen[idx - 1] == length:
                idx -= 1
            return idx
        if plen[idx] > length:
            return idx if begin == idx else bin_search(begin, idx - 1, length)
        return bin_search(idx + 1, last, length)

    lo, hi = [], []
    for ql in qlen:
        s0 = bin_search(0, len(plen) - 1, int(ql * 0.9))
        e0 = s0
        while e0 < len(plen) and plen[e0] <= int(ql / 0.9):
            e0 += 1
        lo.append(s0)
        hi.append(e0)

    def fh(hdr):
        b = 1 if hdr.startswith(">") else 0
        for i in range(b, len(hdr)):
            if hdr[i] in " \t":
                return hdr[b:i + 1]
        return hdr[b:]

    pred = api.Predictor.from_file(ctx, os.path.join(GOLDEN, "weights_k9_u32_fc.txt"))
    offsets, idx, sim, info = pred.search_pairs(dset, np.array(order, dtype=np.uint32), qset, np.arange(len(qs), dtype=np.uint32),
                                                win_lo=lo, win_hi=hi)
    assert info["route"] == api.PAIRS_ROUTE_MATRIX
    out = []
    for j in range(len(qs)):
        for p in range(int(offsets[j]), int(offsets[j + 1])):
            if sim[p] > 0:
                out.append("%s\t%s\t%g\n" % (fh(hq[j]), fh(h[order[idx[p]]]), 100 * sim[p]))
    assert "".join(out).encode() == open(os.path.join(GOLDEN, "fastcar_k9_u32.out"), "rb").read()


def test_scale_1024_by_100000(ctx):
    seqs, _ = synth.families(100, 100000, 1000, family=20)
    hs = _set(ctx, seqs, 9, 32)
    pred = api.Predictor.from_file(ctx, os.path.join(GOLDEN, "weights_k9_u32_fc.txt"))
    q = np.arange(0, 100000, 100000 // 1024, dtype=np.uint32)[:1024]
    offsets, idx, sim, info = pred.search_pairs(hs, None, hs, q, m=len(seqs))
    assert info["route"] == api.PAIRS_ROUTE_MATRIX
    counts = api.score_multi(ctx, pred.cls, hs, None, hs, q, m=len(seqs), want=("close", "counts"))["counts"]
    assert np.array_equal(np.diff(offsets), counts)
    for j in (0, 511, 1023):
        close, s = pred.search(hs, None, hs, int(q[j]), m=len(seqs))
        hit = np.nonzero(close)[0]
        a, b = int(offsets[j]), int(offsets[j + 1])
        assert np.array_equal(idx[a:b], hit), j
        assert np.array_equal(sim[a:b].view(np.uint64), s[hit].view(np.uint64)), j


_CHUNKED = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
from meshclust2_amd import api, synth
from golden_util import weights_text
ctx = api.Context(0)
seqs, _ = synth.families(77, 70000, 1000, family=20)
hs = api.HistogramSet(ctx, 9, 32, len(seqs))
for off in range(0, len(seqs), 4096):
    hs.build(seqs[off:off + 4096], first_slot=off)
pred = api.Predictor.from_text(ctx, weights_text("weights_k9_u32_fc.txt"))
q = np.arange(0, 70000, 350, dtype=np.uint32)
rng = np.random.default_rng(3)
lo = rng.integers(0, 70000, size=q.size).astype(np.uint64)
hi = np.minimum(lo + 40000, 70000).astype(np.uint64)
offsets, idx, sim, info = pred.search_pairs(hs, None, hs, q, win_lo=lo, win_hi=hi, m=len(seqs))
assert info["route"] == api.PAIRS_ROUTE_MATRIX, info
close = api.score_multi(ctx, pred.cls, hs, None, hs, q, m=len(seqs), want=("close",))["close"]
s = np.clip(api.score_multi(ctx, pred.reg, hs, None, hs, q, m=len(seqs), want=("sum",))["sum"], 0.0, 1.0)
for j in range(q.size):
    hit = np.nonzero(close[j, lo[j]:hi[j]])[0] + int(lo[j])
    a, b = int(offsets[j]), int(offsets[j + 1])
    assert np.array_equal(idx[a:b], hit), j
    assert np.array_equal(sim[a:b].view(np.uint64), s[j, hit].view(np.uint64)), j
print("ok", info["n_pairs"])
"""


def test_candidates_in_several_chunks_keep_query_order():
    """With at least 64 slices per product (MSC_GEMM_SLICES, read once per process: a child process) 35 000+ candidates take more than one
    chunk of the product array: each chunk's pairs are staged and gathered query by query."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MSC_GEMM_SLICES="64")
    r = subprocess.run([sys.executable, "-c", _CHUNKED, os.path.dirname(tests), tests], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"ok" in r.stdout, r.stdout.decode(errors="replace")[-3000:]
