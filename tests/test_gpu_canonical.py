"""msc_hist_canonical_batch on the device, and the --canonical switches of msc_cluster and msc_fastcar.

The reference is tests/canonical_util.py (the numpy restatement: rc from the digit rule, the clamped sum, the 1-mers), which test_canonical_cpu.py
holds to the oracle's histograms. Bins are compared exactly; the record is compared with that of a slot filled by msc_hist_upload of the helper's
bins (stddev bit for bit); in-place, out-of-place and mixed batches are compared as raw device bytes.

Shapes: the smallest that reach each kernel form -- padded single tiles (k = 3, 4), the whole-slot LDS kernel (k = 5), the tiled kernel with
uint32_t and with uint64_t bins (k = 9), sparse lists merged in LDS (k = 9, k = 11) and one list past 16 384 entries through the dense scratch slot."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from build_route_check import ID, REC_WORDS, layout
from canonical_util import canon, one_mers, rc_perm, rc_string
from golden_util import EXACT, FEATS, GOLDEN, weights_text
from meshclust2_amd import api, synth
from meshclust2_amd._capi import MscError
from oracle import oracle_py

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_OOM = -1, -4
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
FAST_MASK = sum(1 << b for _, b in FEATS)
DENSE = [(3, 8), (4, 16), (5, 16), (9, 32), (9, 64)]
# A classification model trained on strand-neutral histograms (msc_cluster --canonical --kmer 9 --datatype 32 --id 0.9 --dump on synth.families(777, 300,
# 1000, family=20)): the models trained on plain histograms normalise by the scale of plain counts and call no two canonical points close
CANONICAL_WEIGHTS = "weights_canonical_k9_u32.txt"


def rnd(n, seed):
    return ACGT[np.random.RandomState(seed).randint(0, 4, n)].tobytes()


def twelve(seed):
    """twelve sequences of 300 - 1 200 bases, two of them with runs of N"""
    rs = np.random.RandomState(seed)
    seqs = [rnd(int(rs.randint(300, 1201)), seed * 100 + i) for i in range(12)]
    seqs[3] = seqs[3][:200] + b"N" * 37 + seqs[3][200:]
    seqs[8] = b"N" * 25 + seqs[8][:400] + b"N" * 60 + seqs[8][400:]
    return seqs


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def read_dense(ctx, hs, L, slots):
    """-> [(record + tile prefix words with the id cleared, raw slot bytes)] per slot"""
    b, sb, s, ss = hs.device_view()
    assert (sb, ss) == (L.slot_bytes, L.stride)
    out = []
    for i in (int(x) for x in slots):
        rec = ctx.memcpy_to_host(s + i * ss, ss)[:8 * (REC_WORDS + L.S)].copy().view(np.uint64)
        rec[ID] = 0
        out.append((rec, ctx.memcpy_to_host(b + i * sb, sb).copy()))
    return out


def same_dense(a, b, tag):
    assert len(a) == len(b)
    for i, ((ra, wa), (rb, wb)) in enumerate(zip(a, b)):
        assert np.array_equal(ra, rb), (tag, i, "record", ra.tolist(), rb.tolist())
        assert np.array_equal(wa, wb), (tag, i, "raw slot", np.flatnonzero(wa != wb)[:8].tolist())


def read_sparse(ctx, hs, slots):
    """-> the packed bytes of each slot (record, sub-range table, list, cum: all but its place in the arena) with the id cleared"""
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


def info_but(hs, slot, *skip):
    inf = hs.info(slot)
    for s in skip:
        inf.pop(s)
    return inf


# ------------------------------------------------------------------------------------------------------------------ 1. bins and record, dense
@pytest.mark.parametrize("k,bits", DENSE)
def test_dense_bins_and_record(ctx, k, bits):
    L = layout(k, bits)
    seqs = twelve(10 * k + bits)
    n = len(seqs)
    ids = np.arange(n, dtype=np.uint32)
    A = api.HistogramSet(ctx, k, bits, n)
    A.build(seqs)
    src = [A.download(i) for i in range(n)]
    exp = [canon(h, k) for h in src]
    before = read_dense(ctx, A, L, ids)
    out = api.HistogramSet(ctx, k, bits, n)
    out.canonical_batch(ids, A, ids)
    assert ctx.last_kernel_info() == ("k_hist_canonical", 0)
    same_dense(read_dense(ctx, A, L, ids), before, "the source is not written")
    up = api.HistogramSet(ctx, k, bits, n)
    for i in range(n):
        assert np.array_equal(out.download(i), exp[i][0]), (k, bits, i, "bins")
        a = A.info(i)
        up.upload(i, exp[i][0], a["length"], one_mers(a["one_mers"]).tolist())
        got = out.info(i)
        assert got["id"] == a["id"] and got["overflow"] == int(bool(a["overflow"]) or exp[i][1]), (k, bits, i)
        assert info_but(out, i, "id", "overflow") == info_but(up, i, "id", "overflow"), (k, bits, i, got, up.info(i))
        assert got["stddev"].hex() == up.info(i)["stddev"].hex()
        assert got["mag"] == got["sum"] == int(exp[i][0].astype(np.uint64).sum())
    # the set's bounds follow the new bins
    _, max_count, max_sum, _ = out.build_info()
    assert max_count == max(int(e[0].max()) for e in exp) and max_sum == max(int(e[0].astype(np.uint64).sum()) for e in exp)
    assert np.array_equal(out.lengths(), A.lengths())
    want = read_dense(ctx, out, L, ids)
    # in place
    B = api.HistogramSet(ctx, k, bits, n)
    B.build(seqs)
    B.canonical_batch(ids, B, ids)
    same_dense(read_dense(ctx, B, L, ids), want, "in place")
    # one batch with both forms: slots 0 .. 5 in place, 6 .. 11 into 12 .. 17
    M = api.HistogramSet(ctx, k, bits, 2 * n)
    M.build(seqs)
    untouched = read_dense(ctx, M, L, ids[6:])
    dst = np.concatenate([ids[:6], ids[6:] + 6]).astype(np.uint32)
    perm = np.random.RandomState(5).permutation(n)
    M.canonical_batch(dst[perm], M, ids[perm])
    same_dense(read_dense(ctx, M, L, dst), want, "mixed batch")
    same_dense(read_dense(ctx, M, L, ids[6:]), untouched, "the sources of the out-of-place half")
    # a slot that is one pair's destination and another's source; a destination named twice: refused, nothing written
    whole = read_dense(ctx, M, L, np.arange(18))
    for d, s in (([1, 2], [2, 0]), ([5, 6], [5, 5]), ([7, 7], [8, 9])):
        with pytest.raises(MscError) as e:
            M.canonical_batch(d, M, s)
        assert e.value.code == ERR_INVALID_ARG, (d, s)
    same_dense(read_dense(ctx, M, L, np.arange(18)), whole, "after the refusals")
    M.canonical_batch([], M, [])          # n == 0


# ------------------------------------------------------------------------------------------------------------------ 2. saturation made by the operator
def test_saturation_made_by_the_operator(ctx):
    k, bits = 3, 8
    hs = api.HistogramSet(ctx, k, bits, 4)
    hs.build([b"A" * 150 + b"C" + b"T" * 150, b"A" * 400 + rnd(50, 1)])
    aaa, ttt = 0, 63
    assert hs.info(0)["overflow"] == 0 and hs.download(0)[aaa] == 149 and hs.download(0)[ttt] == 149
    assert hs.info(1)["overflow"] == 1          # saturated by the build
    hs.canonical_batch([2, 3], hs, [0, 1])
    got = hs.download(2)
    assert got[aaa] == 255 and got[ttt] == 255 and hs.info(2)["overflow"] == 1 and hs.info(2)["max_count"] == 255
    assert np.array_equal(got, canon(hs.download(0), k)[0])
    assert hs.info(3)["overflow"] == 1 and np.array_equal(hs.download(3), canon(hs.download(1), k)[0])
    hs.canonical_batch([0], hs, [0])          # in place: the same flag
    assert hs.info(0)["overflow"] == 1 and np.array_equal(hs.download(0), got)


# ------------------------------------------------------------------------------------------------------------------ 3. strand invariance
@pytest.mark.parametrize("sparse", [False, True])
def test_a_sequence_and_its_reverse_complement_are_one_point(ctx, sparse):
    k, bits = 9, 32
    seqs = [rnd(900 + 61 * i, 300 + i) for i in range(6)]
    ent = 4 * sum(len(s) for s in seqs) if sparse else 0
    F = api.HistogramSet(ctx, k, bits, 6, sparse_entries=ent)
    R = api.HistogramSet(ctx, k, bits, 6, sparse_entries=ent)
    F.build(seqs)
    R.build([rc_string(s) for s in seqs])
    ids = np.arange(6, dtype=np.uint32)
    F.canonical_batch(ids, F, ids)
    R.canonical_batch(ids, R, ids)
    for i in range(6):
        assert np.array_equal(F.download(i), R.download(i)), i
        assert info_but(F, i, "id") == info_but(R, i, "id"), i
    if sparse:
        for x, y in zip(read_sparse(ctx, F, ids), read_sparse(ctx, R, ids)):
            assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ 4. sparse
def _oracle_hist(bins, k, bits, length, om):
    """an oracle histogram that holds the given bins (built from a string, then overwritten)"""
    h = oracle_py.hist(b"ACGT" * 10, k, bits)
    bins = np.ascontiguousarray(bins)
    C.memmove(h.bins, bins.ctypes.data, bins.nbytes)
    h.mag = int(bins.astype(np.uint64).sum())
    h.length = int(length)
    h.stddev = float(np.sqrt(np.mean((bins.astype(np.float64) - bins.astype(np.float64).mean()) ** 2)))
    for i in range(4):
        h.one_mers[i] = int(om[i])
    return h


@pytest.mark.parametrize("k,bits", [(9, 32), (11, 16)])
def test_sparse_lists(ctx, k, bits):
    seqs = twelve(1000 + k)[:8]
    seqs[5] = b"G" * 70000 if bits == 16 else seqs[5]          # k = 11 / uint16_t: a bin the build saturates
    n = len(seqs)
    ids = np.arange(n, dtype=np.uint32)
    ent = sum(len(s) for s in seqs)
    A = api.HistogramSet(ctx, k, bits, n, sparse_entries=ent)
    A.build(seqs)
    src = [A.download(i) for i in range(n)]
    exp = [canon(h, k) for h in src]
    p = rc_perm(k)
    union = [int(((h != 1) | (h[p] != 1)).sum()) for h in src]
    out = api.HistogramSet(ctx, k, bits, n, sparse_entries=sum(union))          # exactly the room the lists need
    out.canonical_batch(ids, A, ids)
    assert ctx.last_kernel_info() == ("k_sparse_canonical_sort", 0)
    for i in range(n):
        assert np.array_equal(out.download(i), exp[i][0]), (k, bits, i)
        assert out.entries(i) == union[i], (k, bits, i)
        got, a = out.info(i), A.info(i)
        s, sq = int(exp[i][0].astype(np.uint64).sum()), int((exp[i][0].astype(np.uint64) ** 2).sum())
        assert (got["sum"], got["mag"], got["sum_sq"], got["max_count"]) == (s, s, sq, int(exp[i][0].max())), (k, bits, i)
        assert (got["length"], got["id"], got["one_mers"]) == (a["length"], a["id"], one_mers(a["one_mers"]).tolist())
        assert got["overflow"] == int(bool(a["overflow"]) or exp[i][1])
    assert out.build_info()[3] == max(union)
    want = read_sparse(ctx, out, ids)
    # in place: the same slots, the old lists left behind in the arena
    B = api.HistogramSet(ctx, k, bits, n, sparse_entries=ent + sum(union))
    B.build(seqs)
    B.canonical_batch(ids, B, ids)
    for x, y in zip(read_sparse(ctx, B, ids), want):
        assert np.array_equal(x, y)
    # an arena one entry too small takes nothing
    small = api.HistogramSet(ctx, k, bits, n, sparse_entries=sum(union) - 1)
    small.canonical_batch([0], A, [0])
    kept = read_sparse(ctx, small, ids)
    with pytest.raises(MscError) as e:
        small.canonical_batch(ids, A, ids)
    assert e.value.code == ERR_OOM
    assert [small.entries(i) for i in range(n)] == [union[0]] + [0] * (n - 1)
    for x, y in zip(read_sparse(ctx, small, ids), kept):
        assert np.array_equal(x, y)
    if k != 9:
        return
    # the statistics of canonical sparse slots: those of canonical dense slots and of the oracle on the downloaded bins
    D = api.HistogramSet(ctx, k, bits, n)
    D.build(seqs)
    D.canonical_batch(ids, D, ids)
    oh = [_oracle_hist(exp[i][0], k, bits, out.info(i)["length"], out.info(i)["one_mers"]) for i in range(n)]
    try:
        for q in (0, 3, n - 1):
            a = api.pair_features_raw(ctx, out, ids, out, q, FAST_MASK)
            b = api.pair_features_raw(ctx, D, ids, D, q, FAST_MASK)
            for c, (name, bit) in enumerate(FEATS):
                if name in EXACT:
                    assert np.array_equal(a[:, c], b[:, c]), (name, q)
                else:
                    assert np.allclose(a[:, c], b[:, c], rtol=1e-9, atol=1e-13), (name, q)
                for j in range(n):
                    ref = oracle_py.raw_feature(1 << bit, oh[j], oh[q])
                    if name in EXACT and name != "kulczynski2":
                        assert a[j, c] == ref, (name, j, q)
                    else:
                        assert a[j, c] == pytest.approx(ref, rel=1e-9, abs=1e-13), (name, j, q)
    finally:
        for h in oh:
            oracle_py.lib().orc_hist_free(h)


def test_a_long_sparse_list_goes_through_the_scratch_slot(ctx):
    k, bits = 9, 32
    seqs = [rnd(40000, 71), rnd(800, 72)]
    A = api.HistogramSet(ctx, k, bits, 2, sparse_entries=300000)
    A.build(seqs)
    assert A.entries(0) > 16384
    A.set_id(0, 77)
    src = A.download(0)
    exp, ovf = canon(src, k)
    p = rc_perm(k)
    before = A.info(0)
    A.canonical_batch([1], A, [1])
    assert ctx.last_kernel_info() == ("k_sparse_canonical_sort", 0)
    A.canonical_batch([0], A, [0])
    assert ctx.last_kernel_info() == ("k_sparse_canonical_scratch", 0)
    assert np.array_equal(A.download(0), exp) and A.entries(0) == int(((src != 1) | (src[p] != 1)).sum())
    got = A.info(0)
    s = int(exp.astype(np.uint64).sum())
    assert (got["sum"], got["mag"], got["max_count"], got["length"], got["id"]) == (s, s, int(exp.max()), before["length"], 77)
    assert got["one_mers"] == one_mers(before["one_mers"]).tolist() and got["overflow"] == int(bool(before["overflow"]) or ovf)
    # the same slot as the dense kernel and the builder's compaction give it
    D = api.HistogramSet(ctx, k, bits, 1)
    D.build(seqs[:1])
    D.canonical_batch([0], D, [0])
    assert info_but(D, 0, "id") == info_but(A, 0, "id")


# ------------------------------------------------------------------------------------------------------------------ 5. mirrors
def test_mirrors_follow_the_new_bins(ctx):
    k, bits = 9, 32
    seqs, _ = synth.families(4242, 190, 1000, family=20, sub_rate=0.01)
    n, m = len(seqs), 130
    pred = api.Predictor.from_text(ctx, weights_text(CANONICAL_WEIGHTS))
    hs = api.HistogramSet(ctx, k, bits, n)
    for off in range(0, n, 64):
        hs.build(seqs[off:off + 64], first_slot=off)
    db, q = np.arange(m, dtype=np.uint32), np.arange(m, n, dtype=np.uint32)
    first = pred.search_pairs(hs, db, hs, q)
    assert first[3]["route"] == api.PAIRS_ROUTE_MATRIX, first[3]
    src = [(hs.download(i), hs.info(i)) for i in range(n)]
    ids = np.arange(n, dtype=np.uint32)
    hs.canonical_batch(ids, hs, ids)
    got = pred.search_pairs(hs, db, hs, q)
    assert got[3]["route"] == api.PAIRS_ROUTE_MATRIX, got[3]
    fresh = api.HistogramSet(ctx, k, bits, n)
    for i, (h, inf) in enumerate(src):
        fresh.upload(i, canon(h, k)[0], inf["length"], one_mers(inf["one_mers"]).tolist())
    exp = pred.search_pairs(fresh, db, fresh, q)
    assert exp[3]["route"] == api.PAIRS_ROUTE_MATRIX, exp[3]
    assert exp[3]["n_pairs"] > 0
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert np.array_equal(got[2].view(np.uint64), exp[2].view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------ 6. msc_cluster --canonical
def _exe(name):
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    exe = os.path.join(host, name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module")
def fasta_pair(tmp_path_factory):
    """A: 300 sequences in families of 20; B: the same with every odd record reverse-complemented"""
    d = tmp_path_factory.mktemp("canonical")
    seqs, hdrs = synth.families(20261020, 300, 1000, family=20, sub_rate=0.01)
    synth.write_fasta(str(d / "a.fa"), seqs, hdrs)
    synth.write_fasta(str(d / "b.fa"), [rc_string(s) if i % 2 else s for i, s in enumerate(seqs)], hdrs)
    return d


def _cluster(d, fa, out, *flags):
    r = subprocess.run([_exe("msc_cluster"), fa, "--output", out] + list(flags), cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    return open(str(d / out), "rb").read()


@pytest.mark.parametrize("layout_flag", [(), ("--sparse",)])
def test_cluster_canonical_does_not_see_the_orientation(fasta_pair, layout_flag):
    w = ("--recover", os.path.join(GOLDEN, CANONICAL_WEIGHTS))
    tag = "sp" if layout_flag else "de"
    a = _cluster(fasta_pair, "a.fa", "a_%s.clstr" % tag, "--canonical", *w, *layout_flag)
    b = _cluster(fasta_pair, "b.fa", "b_%s.clstr" % tag, "--canonical", *w, *layout_flag)
    assert a == b and a.count(b">Cluster") > 0
    if not layout_flag:
        # B without the flag: a family falls into one cluster per orientation. That run takes the committed model trained on plain histograms --
        # a model goes with the kind of histogram it was trained on: under the canonical model every plain histogram, at half the scale, is close
        # to every other (measured: 1 cluster), and under the plain model no two canonical ones are
        plain = _cluster(fasta_pair, "b.fa", "b_plain.clstr", "--recover", os.path.join(GOLDEN, "weights_k9_u32.txt"))
        print("clusters of B: %d with --canonical, %d without" % (b.count(b">Cluster"), plain.count(b">Cluster")))
        assert plain.count(b">Cluster") > b.count(b">Cluster")


def test_cluster_canonical_trains_the_same_model_on_both_orientations(fasta_pair):
    _cluster(fasta_pair, "a.fa", "a_tr.clstr", "--canonical", "--dump", "wa.txt")
    _cluster(fasta_pair, "b.fa", "b_tr.clstr", "--canonical", "--dump", "wb.txt")
    wa, wb = open(str(fasta_pair / "wa.txt"), "rb").read(), open(str(fasta_pair / "wb.txt"), "rb").read()
    assert wa == wb and b"n_combos:" in wa


# ------------------------------------------------------------------------------------------------------------------ 7. msc_fastcar --canonical
@pytest.mark.parametrize("flags", [(), ("--top", "3"), ("--sparse",), ("--sparse", "--sparse-matrix")])
def test_fastcar_canonical_gives_a_query_and_its_reverse_complement_the_same_lines(tmp_path, flags):
    db, h = synth.families(5151, 200, 1000, family=20, sub_rate=0.01)
    q = [db[i][:len(db[i]) - 5] for i in range(0, 200, 5)]
    hq = [">q%d" % i for i in range(len(q))]
    synth.write_fasta(str(tmp_path / "db.fa"), db, h)
    synth.write_fasta(str(tmp_path / "q.fa"), q, hq)
    synth.write_fasta(str(tmp_path / "qrc.fa"), [rc_string(s) for s in q], hq)
    outs = []
    for query in ("q.fa", "qrc.fa"):
        r = subprocess.run([_exe("msc_fastcar"), "db.fa", "--query", query, "--recover", os.path.join(GOLDEN, CANONICAL_WEIGHTS), "--output", "o_" + query, "--canonical"]
                           + list(flags), cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
        outs.append(open(str(tmp_path / ("o_" + query + "0")), "rb").read())
    assert outs[0] == outs[1] and outs[0].count(b"\n") > 0
