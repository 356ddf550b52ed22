"""msc_hist_revcomp_batch: the reverse complement of slots as a permutation of their bins, on the device.

The reference is the project's own builder on the reverse-complement STRINGS (the builder suites hold it to the oracle): set A is built from s,
set B from rc(s), set C is revcomp_batch of A into the same slot numbers. C and B are compared as raw device bytes per slot, read as
build_route_check.py reads them: the tile-permuted slot, the 128-byte record (every word but `id`), the S tile prefixes, download(); for sparse
sets the packed slot of msc_hist_pack (record, sub-range table, list, cum). download() of C is also held to the oracle's histogram of rc(s).
No tolerance anywhere: the operator copies counts.

Shapes: the smallest at which a kernel can go wrong -- padded single tiles (k <= 4), LPT 1 / 2 / 4, the whole-slot LDS kernel up to its 64 KiB
limit and the tiled kernel from the first shape past it, the 512-bin uint64_t tile, 256 tiles at even and odd k, 16 MiB slots; sparse lists
sorted in LDS (one of exactly 32 768 entries) and one past that through the dense scratch slot."""
import numpy as np
import pytest

from build_route_check import ID, REC_WORDS, layout, up16
from meshclust2_amd import api, synth
from meshclust2_amd._capi import MscError
from oracle import oracle_py

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_OOM = -1, -4
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

DENSE = [(1, 32), (2, 32), (3, 32), (4, 8), (5, 8), (5, 16), (5, 32), (6, 8), (7, 16), (8, 8), (8, 16), (8, 64), (9, 32), (10, 8), (12, 8)]
SPARSE = [(8, 32), (9, 32), (11, 8), (13, 64), (15, 8)]


def rc(s):
    return s.translate(_COMP)[::-1]


def rnd(n, seed):
    return ACGT[np.random.RandomState(seed).randint(0, 4, n)].tobytes()


def distinct_prefix(seq, k, want):
    """the shortest prefix of seq with `want` distinct k-mers"""
    c = np.frombuffer(seq, dtype=np.uint8).copy()
    codes = np.zeros(256, dtype=np.int64)
    codes[ACGT] = np.arange(4)
    c = codes[c]
    n = c.size - k + 1
    idx = np.zeros(n, dtype=np.int64)
    for j in range(k):
        idx = idx * 4 + c[j:j + n]
    _, first = np.unique(idx, return_index=True)
    first.sort()
    return seq[:int(first[want - 1]) + k]


def sequences(k, bits, sparse):
    if (k, bits) == (12, 8):          # 16 MiB slots: four of them
        return [rnd(3000, 1), b"A" * 200, b"", rnd(300, 2)]
    half = rnd(max(k // 2, 1), 77)
    pal = half + rc(half)             # an even palindrome: its own reverse complement
    seqs = [b"", rnd(k - 1, 3), rnd(k, 4), rnd(k + 1, 5), rnd(300, 6), rnd(3000, 7), rnd(3000, 8),
            b"A" * 200,               # bin 0 <-> bin 4^k - 1
            pal * 40, b"ACGT" * 60, b"AATT" * 60,
            # one k-mer 254 / 255 / 256 times: the last value a uint8_t bin holds, then saturation with the overflow flag
            b"C" * (k - 1 + 254), b"C" * (k - 1 + 255), b"C" * (k - 1 + 256), rnd(100, 9) + b"G" * (k + 300) + rnd(100, 10)]
    seqs += [rnd(500 + 97 * i, 20 + i) for i in range(24 - len(seqs))]
    if sparse and k == 13:
        seqs.append(rnd(40000, 11))                              # a list past 32 768 entries: the scratch route
        seqs.append(distinct_prefix(rnd(34000, 12), k, 32768))   # exactly 32 768 entries: the last list the sort takes
    return seqs


def new_set(ctx, k, bits, n, sparse, entries=0):
    return api.HistogramSet(ctx, k, bits, n, sparse_entries=entries + 64 if sparse else 0)


def build(ctx, k, bits, seqs, sparse, capacity=None):
    hs = new_set(ctx, k, bits, capacity or len(seqs), sparse, sum(len(s) for s in seqs))
    for off in range(0, len(seqs), 8):
        hs.build(seqs[off:off + 8], first_slot=off)
    return hs


def read_dense(ctx, hs, L, slots):
    """-> [(record + prefix words with the id cleared, raw slot bytes)] per slot"""
    b, sb, s, ss = hs.device_view()
    assert (sb, ss) == (L.slot_bytes, L.stride)
    out = []
    for i in (int(x) for x in slots):
        rec = ctx.memcpy_to_host(s + i * ss, ss)[:8 * (REC_WORDS + L.S)].copy().view(np.uint64)
        rec[ID] = 0
        out.append((rec, ctx.memcpy_to_host(b + i * sb, sb).copy()))
    return out


def read_sparse(ctx, hs, slots):
    """-> the packed byte range of each slot (msc_shard.hip: head, record, sub-range table, list, cum) with the id cleared"""
    slots = [int(x) for x in slots]
    sizes = [hs.packed_bytes(s) for s in slots]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    dev = ctx.device_malloc(int(offs[-1]))
    try:
        ctx.memcpy_to_device(dev, np.zeros(int(offs[-1]), dtype=np.uint8))
        hs.pack(slots, dev, offs[:-1])
        img = ctx.memcpy_to_host(dev, int(offs[-1]))
    finally:
        ctx.device_free(dev)
    out = []
    for i in range(len(slots)):
        one = img[int(offs[i]):int(offs[i + 1])].copy()
        one[16 + 8 * ID:16 + 8 * ID + 8] = 0
        out.append(one)
    return out


def same_slots(ctx, got, exp, L, sparse, slots_got, slots_exp, tag):
    if sparse:
        a, b = read_sparse(ctx, got, slots_got), read_sparse(ctx, exp, slots_exp)
        for i, (x, y) in enumerate(zip(a, b)):
            n = got.entries(int(slots_got[i]))
            assert n == exp.entries(int(slots_exp[i])), (tag, i, "entries")
            assert x.size == y.size == 16 + 128 + 80 + up16(8 * n) + up16(4 * n), (tag, i, "packed size")
            assert np.array_equal(x[16:144], y[16:144]), (tag, i, "record", x[16:144].view(np.uint64).tolist(), y[16:144].view(np.uint64).tolist())
            assert np.array_equal(x[144:224], y[144:224]), (tag, i, "sub-range table")
            assert np.array_equal(x[224:224 + up16(8 * n)], y[224:224 + up16(8 * n)]), (tag, i, "list")
            assert np.array_equal(x, y), (tag, i, "cum / head")
        return
    a, b = read_dense(ctx, got, L, slots_got), read_dense(ctx, exp, L, slots_exp)
    for i, ((ra, wa), (rb, wb)) in enumerate(zip(a, b)):
        assert np.array_equal(ra[:REC_WORDS], rb[:REC_WORDS]), (tag, i, "record", ra[:REC_WORDS].tolist(), rb[:REC_WORDS].tolist())
        assert np.array_equal(ra[REC_WORDS:], rb[REC_WORDS:]), (tag, i, "tile prefixes")
        assert np.array_equal(wa, wb), (tag, i, "raw slot", np.flatnonzero(wa != wb)[:8].tolist())


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("k,bits,sparse", [(k, b, False) for k, b in DENSE] + [(k, b, True) for k, b in SPARSE])
def test_revcomp_is_the_builder_on_the_reverse_complement_strings(ctx, k, bits, sparse):
    L = layout(k, bits)
    seqs = sequences(k, bits, sparse)
    n = len(seqs)
    ids = np.arange(n, dtype=np.uint32)
    A = build(ctx, k, bits, seqs, sparse)
    B = build(ctx, k, bits, [rc(s) for s in seqs], sparse)
    C = new_set(ctx, k, bits, n, sparse, sum(len(s) for s in seqs))
    C.revcomp_batch(ids, A, ids)
    name, q_per_read = ctx.last_kernel_info()
    long_lists = sparse and any(A.entries(i) > 32768 for i in range(n))
    assert name == ("k_sparse_revcomp_scratch" if long_lists else "k_sparse_revcomp_sort" if sparse else "k_hist_revcomp") and q_per_read == 0, (name, q_per_read)
    same_slots(ctx, C, B, L, sparse, ids, ids, (k, bits, "C == B"))
    assert np.array_equal(C.lengths(), B.lengths())
    if k <= 10:
        for i in range(n):
            assert np.array_equal(C.download(i), B.download(i)), (k, bits, i, "download")
        for i in (range(n) if k <= 8 else range(0, n, 4)):
            oh = oracle_py.hist(rc(seqs[i]), k, bits)
            try:
                assert np.array_equal(C.download(i), oh.array()), (k, bits, i, "oracle")
            finally:
                oracle_py.lib().orc_hist_free(oh)
    # involution: the reverse complement of C is A again (a sparse slot: all but its place in the arena, which the packed slot does not carry)
    D = new_set(ctx, k, bits, n, sparse, sum(len(s) for s in seqs))
    D.revcomp_batch(ids[::-1].copy(), C, ids[::-1].copy())
    same_slots(ctx, D, A, L, sparse, ids, ids, (k, bits, "D == A"))
    if sparse and k == 13:          # the routes by name: the list of exactly 32 768 entries is sorted, the one past it goes through the scratch slot
        assert A.entries(n - 1) == 32768 and A.entries(n - 2) > 32768
        E = new_set(ctx, k, bits, 2, True, 80000)
        E.revcomp_batch([0], A, [n - 1])
        assert ctx.last_kernel_info() == ("k_sparse_revcomp_sort", 0)
        E.revcomp_batch([1], A, [n - 2])
        assert ctx.last_kernel_info() == ("k_sparse_revcomp_scratch", 0)
        same_slots(ctx, E, B, L, True, [0, 1], [n - 1, n - 2], "routes")


@pytest.mark.parametrize("k,bits,sparse", [(5, 16, False), (9, 32, False), (8, 32, True)])
def test_a_stale_mag_stays_and_a_set_serves_itself(ctx, k, bits, sparse):
    L = layout(k, bits)
    seqs = [rnd(700, 31), rnd(900, 32), rnd(800, 33)]
    ent = 4 * sum(len(s) for s in seqs)
    A = build(ctx, k, bits, seqs, sparse)
    B = build(ctx, k, bits, [rc(s) for s in seqs], sparse)
    X = new_set(ctx, k, bits, 6, sparse, ent)
    X.build(seqs, first_slot=0)
    X.assign_from(0, A, 1)          # DivergencePoint::set: the bins of s1 under the magnitude of s0
    stale = X.info(0)["mag"]
    assert stale == A.info(0)["mag"] != A.info(1)["mag"]
    X.revcomp_batch([3, 4, 5], X, [0, 1, 2])          # dst == src is legal while no slot is both
    assert X.info(3)["mag"] == stale
    assert X.info(3)["one_mers"] == X.info(0)["one_mers"][::-1]
    for what in ("length", "sum", "sum_sq", "max_count", "stddev", "overflow"):
        assert X.info(3)[what] == X.info(0)[what], what
    if k <= 10:
        assert np.array_equal(X.download(3), B.download(1))
    same_slots(ctx, X, B, L, sparse, [4, 5], [1, 2], "same set")
    # a slot that is a source and a destination: refused, nothing written
    before = read_sparse(ctx, X, list(range(6))) if sparse else read_dense(ctx, X, L, list(range(6)))
    with pytest.raises(MscError) as e:
        X.revcomp_batch([1, 2], X, [2, 0])
    assert e.value.code == ERR_INVALID_ARG
    with pytest.raises(MscError) as e:
        X.revcomp_batch([4, 4], A, [0, 1])          # a destination named twice
    assert e.value.code == ERR_INVALID_ARG
    after = read_sparse(ctx, X, list(range(6))) if sparse else read_dense(ctx, X, L, list(range(6)))
    for x, y in zip(before, after):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)) if isinstance(x, tuple) else np.array_equal(x, y)


def test_argument_rules_are_copy_batchs(ctx):
    a = api.HistogramSet(ctx, 5, 16, 4)
    b = api.HistogramSet(ctx, 5, 16, 4)
    a.build([rnd(200, 41), rnd(300, 42)])
    b.revcomp_batch([], a, [])          # n == 0
    for dst, d, src, s in ((b, [4], a, [0]), (b, [0], a, [4]), (api.HistogramSet(ctx, 5, 32, 4), [0], a, [0]), (api.HistogramSet(ctx, 6, 16, 4), [0], a, [0])):
        with pytest.raises(MscError) as e:
            dst.revcomp_batch(d, src, s)
        assert e.value.code == ERR_INVALID_ARG
    sp = api.HistogramSet(ctx, 8, 16, 4, sparse_entries=1000)
    with pytest.raises(MscError) as e:
        sp.revcomp_batch([0], api.HistogramSet(ctx, 8, 16, 4), [0])          # layouts differ
    assert e.value.code == ERR_INVALID_ARG


def test_a_sparse_arena_too_small_takes_nothing(ctx):
    k, bits = 9, 32
    seqs = [rnd(600, 51), rnd(700, 52), rnd(800, 53)]
    A = build(ctx, k, bits, seqs, True)
    need = sum(A.entries(i) for i in range(3))
    C = api.HistogramSet(ctx, k, bits, 3, sparse_entries=need - 1)
    with pytest.raises(MscError) as e:
        C.revcomp_batch([0, 1, 2], A, [0, 1, 2])
    assert e.value.code == ERR_OOM
    assert [C.entries(i) for i in range(3)] == [0, 0, 0]
    # nothing was appended: the two lists that fit the arena still do, to the last entry
    small = sorted(range(3), key=A.entries)[:2]
    fits = api.HistogramSet(ctx, k, bits, 3, sparse_entries=sum(A.entries(i) for i in small))
    with pytest.raises(MscError):
        fits.revcomp_batch([0, 1, 2], A, [0, 1, 2])
    fits.revcomp_batch(small, A, small)
    B = build(ctx, k, bits, [rc(s) for s in seqs], True)
    same_slots(ctx, fits, B, layout(k, bits), True, small, small, "after the refusal")


@pytest.mark.parametrize("sparse", [False, True])
def test_mirrors_follow_the_new_bins(ctx, sparse):
    """kb / mb / ranks exist before the call; afterwards the matrix-core pass scores the new contents bit for bit as a freshly built set does"""
    from golden_util import weights_text
    k, bits = 9, 32
    seqs, _ = synth.families(6161, 140, 1000, family=20, sub_rate=0.01, indel_rate=0.002)
    n = len(seqs)
    feat = api.Feature.from_text(ctx, weights_text("weights_k9_u32_fc.txt"), 0)
    ctx.set_sparse_matrix_pass(sparse)
    try:
        hs = api.HistogramSet(ctx, k, bits, n, sparse_entries=2 * sum(len(s) for s in seqs) if sparse else 0)          # (room in the arena for the 40 new lists)
        for off in range(0, n, 70):
            hs.build(seqs[off:off + 70], first_slot=off)
        src = build(ctx, k, bits, seqs, sparse)
        q = np.arange(0, n, 2, dtype=np.uint32)
        api.score_multi(ctx, feat, hs, None, hs, q, m=n)
        assert ctx.last_kernel_info()[0].startswith("k_pair_gemm_fp4_dma<"), ctx.last_kernel_info()
        turned = np.arange(3, 123, 3, dtype=np.uint32)          # 40 slots
        hs.revcomp_batch(turned, src, turned)
        got = api.score_multi(ctx, feat, hs, None, hs, q, m=n)
        assert ctx.last_kernel_info()[0].startswith("k_pair_gemm_fp4_dma<"), ctx.last_kernel_info()
        which = set(turned.tolist())
        now = [rc(s) if i in which else s for i, s in enumerate(seqs)]
        fresh = build(ctx, k, bits, now, sparse)
        exp = api.score_multi(ctx, feat, fresh, None, fresh, q, m=n)
        assert ctx.last_kernel_info()[0].startswith("k_pair_gemm_fp4_dma<"), ctx.last_kernel_info()
        for what in ("sum", "csum", "close"):
            assert np.array_equal(np.asarray(got[what]).view(np.uint8), np.asarray(exp[what]).view(np.uint8)), what
    finally:
        ctx.set_sparse_matrix_pass(False)
