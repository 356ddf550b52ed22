"""msc_align_pairs_banded and msc_align_pairs_auto on the device, and msc_fastcar --align --align-band.

The banded triple and its flag are held, exactly, to tests/align_band_util.py -- the numpy restatement of the banded operator and of the
certificate that tests/test_align_band_cpu.py holds to the unbanded restatement and, for soundness, to an exhaustive search -- and every
certified triple to the reference's own integers (tests/golden/align_pairs.npz) or to msc_align_pairs run on the device in the same test.
msc_align_pairs_auto is held to msc_align_pairs, bit for bit, and its band_used to the restatement's doubling sequence."""
import os
import subprocess

import numpy as np
import pytest

import align_band_util
import align_util
from meshclust2_amd import api, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return align_util.Fixture()


def _quad(r):
    return np.stack([r["score"], r["length"], r["matches"], r["certified"]], axis=1).astype(np.int64)


def _triples(r):
    return np.stack([r["score"], r["length"], r["matches"]], axis=1).astype(np.int64)


def _same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def _mutant(rs, codes, rate):
    """msc_cluster.cpp's recipe: rate * 0.8 substitutions, * 0.1 deletions, * 0.1 insertions per position"""
    out = []
    for c in codes.tolist():
        u = rs.rand()
        if u < rate * 0.8:
            out.append(int(_ACGT[rs.randint(0, 4)]))
        elif u < rate * 0.9:
            continue
        elif u < rate:
            out.extend((c, int(_ACGT[rs.randint(0, 4)])))
        else:
            out.append(c)
    return bytes(out) if out else b"A"


def test_the_fixture_at_six_bands(ctx, fx):
    bands = [0, 1, 7, 64, 300, 40000]
    small = np.nonzero(fx.cells() <= 300 * 300)[0]
    firsts, seconds = [fx.seqs[i] for i in fx.first[small]] * len(bands), [fx.seqs[i] for i in fx.second[small]] * len(bands)
    for s, params in enumerate(fx.params):
        want = align_band_util.banded_many(firsts, seconds, np.repeat(bands, small.size), params).reshape(len(bands), small.size, 4)
        for k, w in enumerate(bands):
            r = api.align_pairs_banded(ctx, fx.seqs, fx.first, fx.second, w, *[int(v) for v in params])
            got = _quad(r)
            assert r["certified"].dtype == np.uint8 and set(np.unique(r["certified"]).tolist()) <= {0, 1}
            _same(got[small], want[k], (params.tolist(), w))
            flag = got[:, 3] == 1
            _same(got[flag, :3], fx.result[s][flag].astype(np.int64), (params.tolist(), w, "certified"))
            if w == 40000:
                assert flag.all()
            assert np.array_equal(r["identity"], r["matches"] / r["length"].astype(np.float64))
    name, per_read = ctx.last_kernel_info()
    assert name.startswith("k_align_band<") and per_read == 0, name


@pytest.fixture(scope="module")
def random_pairs():
    """2 000 pairs of 1 .. 700 bytes (short ones more often than long ones): mutated relatives at 1 - 25 %, unrelated pairs, pieces
    at length ratios up to 1 : 5; a random half-width in 0 .. 200 per pair; eight groups of 250, each under another parameter set drawn from those of
    the soundness test, one of them without a certificate. -> seqs, first, second, bands, [(params, slice)], the restatement's [n, 4]"""
    rs = np.random.RandomState(61)
    seqs, first, second = [], [], []
    for p in range(2000):
        n = int(round(700 ** rs.rand() ** 0.5))
        a = _ACGT[rs.randint(0, 4, max(1, n))]
        kind = p % 4
        if kind == 0:
            b = _ACGT[rs.randint(0, 4, max(1, int(round(700 ** rs.rand() ** 0.5))))].tobytes()          # unrelated
        elif kind == 1:
            cut = max(1, int(a.size / rs.uniform(1, 5)))                                          # a mutated piece: a length ratio up to 1 : 5
            at = int(rs.randint(0, a.size - cut + 1))
            b = _mutant(rs, a[at:at + cut], rs.uniform(0.01, 0.25))
        else:
            b = _mutant(rs, a, rs.uniform(0.01, 0.25))
        pair = (a.tobytes(), b[:700]) if rs.rand() < 0.5 else (b[:700], a.tobytes())
        first.append(len(seqs))
        second.append(len(seqs) + 1)
        seqs.extend(pair)
    bands = rs.randint(0, 201, 2000)
    drawn = [align_band_util.OFFERED[i] for i in rs.permutation(16)[:7]]
    drawn.insert(3, align_band_util.REFUSED[int(rs.randint(0, 3))])          # (one group without a certificate)
    groups = [(drawn[g], slice(250 * g, 250 * (g + 1))) for g in range(8)]
    want = np.zeros((2000, 4), dtype=np.int64)
    for params, sl in groups:
        want[sl] = align_band_util.banded_many([seqs[i] for i in first[sl]], [seqs[i] for i in second[sl]], bands[sl], params, step=128)
    assert max(len(s) for s in seqs) <= 700 and min(len(s) for s in seqs) >= 1
    return seqs, np.array(first, dtype=np.uint32), np.array(second, dtype=np.uint32), bands, groups, want


def test_two_thousand_random_pairs_are_the_restatements(ctx, random_pairs):
    seqs, first, second, bands, groups, want = random_pairs
    certified = 0
    for params, sl in groups:
        full = _triples(api.align_pairs(ctx, seqs, first[sl], second[sl], *params))
        for w in np.unique(bands[sl]):          # (a call has one band: the pairs that drew it)
            idx = np.nonzero(bands[sl] == w)[0] + sl.start
            got = _quad(api.align_pairs_banded(ctx, seqs, first[idx], second[idx], int(w), *params))
            _same(got, want[idx], (params, int(w)))
            flag = got[:, 3] == 1
            _same(got[flag, :3], full[idx - sl.start][flag], (params, int(w), "certified"))
            certified += int(flag.sum())
    assert 200 < certified < 1900, certified


def test_the_edges_of_stripes_windows_and_the_band(ctx):
    rs = np.random.RandomState(62)
    base = _ACGT[rs.randint(0, 4, 760)]
    seqs, first, second = [], [], []
    for la in (1, 255, 256, 257, 513, 700):
        for delta in (-50, -1, 0, 1, 50):
            if la + delta < 1:
                continue
            first.append(len(seqs))
            second.append(len(seqs) + 1)
            seqs.extend((_mutant(rs, base[:la], 0.05)[:la].ljust(la, b"C"), base[5:5 + la + delta].tobytes()))
    for shape in ((1, 300), (300, 1)):
        first.append(len(seqs))
        second.append(len(seqs) + 1)
        seqs.extend((base[:shape[0]].tobytes(), base[200:200 + shape[1]].tobytes()))
    assert [len(seqs[i]) for i in first[:5]] == [1, 1, 1, 255, 255] and len(first) == 30
    bands = [0, 1, 63, 64, 255, 256]
    firsts, seconds = [seqs[i] for i in first] * len(bands), [seqs[i] for i in second] * len(bands)
    for params in ((1, -1, 2, 1), (2, -3, 5, 2)):
        want = align_band_util.banded_many(firsts, seconds, np.repeat(bands, len(first)), params, step=64).reshape(len(bands), len(first), 4)
        for k, w in enumerate(bands):
            _same(_quad(api.align_pairs_banded(ctx, seqs, first, second, w, *params)), want[k], (params, w))
    # a sequence against itself on the main diagonal alone
    for params in ((1, -1, 2, 1), (2, -3, 5, 2)):
        r = api.align_pairs_banded(ctx, seqs, first, first, 0, *params)
        ln = np.array([len(seqs[i]) for i in first])
        assert r["certified"].all() and np.array_equal(r["score"], params[0] * ln) and np.array_equal(r["length"], ln) and np.array_equal(r["matches"], ln)


def test_a_long_pair_whose_carry_ring_leaves_lds(ctx):
    """20 000 bytes against a 3 % mutant at half-width 2 600: about 40 KiB of sequences and a ring of some 5 460 rows of 24 bytes (128 KiB)
    exceed a workgroup's 160 KiB, so the ring lives in global memory; at 1 024 it fits"""
    rs = np.random.RandomState(63)
    a = _ACGT[rs.randint(0, 4, 20000)]
    seqs = [a.tobytes(), _mutant(rs, a, 0.03)]
    full = _triples(api.align_pairs(ctx, seqs, [0, 1], [1, 0]))
    for w, where in ((2600, "global memory"), (1024, "LDS")):
        r = api.align_pairs_banded(ctx, seqs, [0, 1], [1, 0], w)
        assert ctx.last_kernel_info()[0] == "k_align_band<4 columns a lane, carry in %s>" % where, ctx.last_kernel_info()
        assert r["certified"].all()
        _same(_triples(r), full, w)


@pytest.fixture(scope="module")
def templates():
    rs = np.random.RandomState(64)
    return rs, [_ACGT[rs.randint(0, 4, 600)] for _ in range(64)]


def test_the_flags_on_mutants_at_three_settings(ctx, templates):
    rs, tpl = templates
    for rate, w, most in ((0.03, 32, True), (0.10, 64, True), (0.10, 32, False)):
        seqs, idx = [], np.arange(64, dtype=np.uint32)
        for t in tpl:
            seqs.extend((t.tobytes(), _mutant(rs, t, rate)))
        for params in ((1, -1, 2, 1), (2, -3, 5, 2)):
            want = align_band_util.banded_many(seqs[0::2], seqs[1::2], w, params, step=1024)
            r = api.align_pairs_banded(ctx, seqs, 2 * idx, 2 * idx + 1, w, *params)
            _same(_quad(r), want, (rate, w, params))
            if most:
                assert r["certified"].sum() * 10 >= 9 * 64, (rate, w, params, int(r["certified"].sum()))


def test_auto_is_msc_align_pairs(ctx, fx, random_pairs):
    # the fixture, every parameter set, three first bands; then reversed and with repeats
    for s, params in enumerate(fx.params):
        p = [int(v) for v in params]
        for first_band in (0, 1, 1000):
            r = api.align_pairs_auto(ctx, fx.seqs, fx.first, fx.second, *p, first_band=first_band)
            _same(_triples(r), fx.result[s].astype(np.int64), (p, first_band))
            assert r["band_used"].dtype == np.uint32
    first, second = np.repeat(fx.first[::-1], 2), np.repeat(fx.second[::-1], 2)
    r = api.align_pairs_auto(ctx, fx.seqs, first, second)
    _same(_triples(r), np.repeat(fx.result[0][::-1], 2, axis=0).astype(np.int64), "reversed")
    assert np.array_equal(r["band_used"][0::2], r["band_used"][1::2])
    small = np.nonzero(fx.cells() <= 300 * 300)[0]
    for first_band in (0, 1):
        r = api.align_pairs_auto(ctx, fx.seqs, fx.first[small], fx.second[small], first_band=first_band)
        want = align_band_util.auto_bands([fx.seqs[i] for i in fx.first[small]], [fx.seqs[i] for i in fx.second[small]], (1, -1, 2, 1), first_band)
        assert np.array_equal(r["band_used"].astype(np.int64), want), first_band
    # the random pairs, each group under its own parameter set (one of them offers no certificate)
    seqs, first, second, _, groups, _ = random_pairs
    banded = 0
    for g, (params, sl) in enumerate(groups):
        full = _triples(api.align_pairs(ctx, seqs, first[sl], second[sl], *params))
        first_band = (0, 1, 1000)[g % 3]
        r = api.align_pairs_auto(ctx, seqs, first[sl], second[sl], *params, first_band=first_band)
        _same(_triples(r), full, (params, first_band))
        want = align_band_util.auto_bands([seqs[i] for i in first[sl]], [seqs[i] for i in second[sl]], params, first_band)
        assert np.array_equal(r["band_used"].astype(np.int64), want), (params, first_band)
        if not align_band_util.offered(params):
            assert (want == align_band_util.NO_BAND).all()
        banded += int((want != align_band_util.NO_BAND).sum())
    assert banded > 50, banded
    # long similar pairs do get a band, and the kernel named is the banded one
    rs = np.random.RandomState(65)
    a = _ACGT[rs.randint(0, 4, 3000)]
    long_seqs = [a.tobytes(), _mutant(rs, a, 0.03), _mutant(rs, a, 0.10), _ACGT[rs.randint(0, 4, 3000)].tobytes()]
    full = _triples(api.align_pairs(ctx, long_seqs, [0, 0, 0, 1], [1, 2, 3, 0]))
    r = api.align_pairs_auto(ctx, long_seqs, [0, 0, 0, 1], [1, 2, 3, 0])
    _same(_triples(r), full, "long")
    assert ctx.last_kernel_info()[0].startswith("k_align_band<")
    assert r["band_used"][3] == r["band_used"][0] < r["band_used"][1] < 0xffffffff == r["band_used"][2], r["band_used"]


def test_an_empty_list_and_the_refusals(ctx, fx):
    for call, last, kw in ((api.align_pairs_banded, np.uint8, dict(band=4)), (api.align_pairs_auto, np.uint32, dict(first_band=4))):
        r = call(ctx, fx.seqs, [], [], **kw)
        assert r["score"].size == 0 and r["identity"].size == 0
        assert call(ctx, [], [], [], **kw)["length"].size == 0

        def refused(seqs, first, second, params=(1, -1, 2, 1)):
            out = tuple(np.full(len(first), -7, dtype=np.int32) for _ in range(3)) + (np.full(len(first), 9, dtype=last),)
            with pytest.raises(api.MscError) as e:
                call(ctx, seqs, first, second, out=out, match=params[0], mismatch=params[1], gap_open=params[2], gap_continue=params[3], **kw)
            assert e.value.code == -1, e.value          # MSC_ERR_INVALID_ARG
            assert all((o == -7).all() for o in out[:3]) and (out[3] == 9).all(), "a refused call wrote an output"

        ok = [b"ACGT", b"AC"]
        refused(ok + [b""], [0, 2], [1, 1])                       # a length of 0
        refused(ok + [b"A" * 32768], [0, 0], [1, 2])              # a length of 32 768
        refused(ok, [0, 1], [1, 2])                               # an index past n_seqs
        for at in range(4):                                       # a parameter of 101 (and of -101)
            for v in (101, -101):
                params = [1, -1, 2, 1]
                params[at] = v
                refused(ok, [0, 1], [1, 0], params)
        # an unlisted sequence may be anything; the limits themselves are legal
        r = call(ctx, ok + [b"", b"A" * 32768], [0], [1], match=100, mismatch=-100, gap_open=100, gap_continue=100, **kw)
        assert _triples(r).tolist() == [list(align_util.align(ok[0], ok[1], (100, -100, 100, 100)))]


def _fastcar(tmp_path, weights, extra, prefix):
    exe = os.path.join(ROOT, "meshclust2_amd", "host", "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "meshclust2_amd", "host")])
    r = subprocess.run([exe, "db.fa", "--query", "q.fa", "--recover", os.path.join(GOLDEN, weights), "--output", prefix] + extra, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-2000:]
    return open(str(tmp_path / (prefix + "0")), "rb").read(), r.stderr.decode()


def test_fastcar_align_band_writes_the_bytes_of_align(tmp_path):
    """the inputs of tests/test_gpu_align.py's two driver tests"""
    db, h = synth.families(41, 300, 1000, family=10, length_jitter=150)
    q, hq = synth.families(41, 40, 1000, family=10, length_jitter=150)
    q = [x[:len(x) - 7] for x in q]
    synth.write_fasta(str(tmp_path / "db.fa"), db, h)
    synth.write_fasta(str(tmp_path / "q.fa"), q, [x.replace(">seq", ">qry") for x in hq])
    plain, _ = _fastcar(tmp_path, "weights_k5_u16.txt", ["--align"], "plain")
    got, err = _fastcar(tmp_path, "weights_k5_u16.txt", ["--align", "--align-band", "8", "--kernels"], "banded")
    assert got == plain and len(plain.splitlines()) > 100
    assert "kernel: k_align_band<" in err, err
    kw = dict(family=4, length_jitter=120, sub_rate=0.01, indel_rate=0.002)
    db, h = synth.families(43, 24, 1000, **kw)
    q, hq = synth.families(43, 8, 1000, **kw)
    q = [x[:len(x) - 5] for x in q]
    q = [x[::-1].translate(_COMP) if i % 2 else x for i, x in enumerate(q)]
    synth.write_fasta(str(tmp_path / "db.fa"), db, h)
    synth.write_fasta(str(tmp_path / "q.fa"), q, [x.replace(">seq", ">qry") for x in hq])
    plain, _ = _fastcar(tmp_path, "weights_k9_u32_fc.txt", ["--both-strands", "--align"], "plain_strands")
    got, _ = _fastcar(tmp_path, "weights_k9_u32_fc.txt", ["--both-strands", "--align", "--align-band", "8"], "banded_strands")
    assert got == plain and len(plain.splitlines()) > 8 and b"\t-\t" in plain
