"""msc_align_pairs on the device, and msc_fastcar --align.

The operator is held to the reference's own integers (tests/golden/align_pairs.npz: every pair, every parameter set, one call per set, exact) and,
for pairs the fixture cannot hold, to tests/align_util.py, the numpy restatement that tests/test_align_cpu.py holds to the same fixture. The
driver's column is held to align_util on the inputs of the k = 5 / 16-bit fastcar fixture."""
import os
import subprocess

import numpy as np
import pytest

import align_util
from meshclust2_amd import api, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return align_util.Fixture()


def _triples(r):
    return np.stack([r["score"], r["length"], r["matches"]], axis=1)


def test_every_fixture_pair_under_every_parameter_set_is_the_references(ctx, fx):
    for s, params in enumerate(fx.params):
        r = api.align_pairs(ctx, fx.seqs, fx.first, fx.second, *[int(v) for v in params])
        got = _triples(r)
        bad = np.nonzero((got != fx.result[s]).any(axis=1))[0]
        assert bad.size == 0, (params.tolist(), int(bad[0]), len(fx.seqs[fx.first[bad[0]]]), len(fx.seqs[fx.second[bad[0]]]), got[bad[0]].tolist(), fx.result[s][bad[0]].tolist())
        assert r["identity"].dtype == np.float64 and np.array_equal(r["identity"], fx.result[s][:, 2] / fx.result[s][:, 1].astype(np.float64))
        assert r["score"].dtype == np.int32
    name, per_read = ctx.last_kernel_info()
    assert name.startswith("k_align_pairs<") and per_read == 0, name


def test_the_list_reversed_and_repeated_comes_back_in_the_callers_order(ctx, fx):
    first = np.repeat(fx.first[::-1], 2)
    second = np.repeat(fx.second[::-1], 2)
    got = _triples(api.align_pairs(ctx, fx.seqs, first, second))
    assert np.array_equal(got, np.repeat(fx.result[0][::-1], 2, axis=0))
    # two calls on one context: the same bytes
    again = _triples(api.align_pairs(ctx, fx.seqs, first, second))
    assert got.tobytes() == again.tobytes()
    # str and bytes are the same sequences
    few = api.align_pairs(ctx, [s.decode() for s in fx.seqs[:12]], [0, 3, 11], [11, 4, 5], 2, -3, 5, 2)
    same = api.align_pairs(ctx, fx.seqs[:12], [0, 3, 11], [11, 4, 5], 2, -3, 5, 2)
    assert np.array_equal(_triples(few), _triples(same))


def test_three_thousand_random_pairs_are_the_restatements(ctx):
    """80 .. 300 bytes, related and unrelated: many short pairs dealt over the grid beside each other"""
    rs = np.random.RandomState(20)
    seqs = []
    for i in range(600):
        n = int(rs.randint(80, 301))
        if i % 3 and seqs:          # a mutated piece of an earlier one
            src = np.frombuffer(seqs[int(rs.randint(0, len(seqs)))], dtype=np.uint8)
            codes = np.resize(src, n).copy()
            hit = rs.rand(n) < 0.08
            codes[hit] = np.frombuffer(b"ACGTN", dtype=np.uint8)[rs.randint(0, 5, int(hit.sum()))]
            codes = np.delete(codes, rs.randint(0, n, 3))
            seqs.append(codes.tobytes() + b"ACGT"[:max(0, 80 - codes.size)])
        else:
            seqs.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, n)].tobytes())
    first = rs.randint(0, len(seqs), 3000).astype(np.uint32)
    second = rs.randint(0, len(seqs), 3000).astype(np.uint32)
    assert min(len(s) for s in seqs) >= 80 and max(len(s) for s in seqs) <= 300
    want = align_util.align_many([seqs[i] for i in first], [seqs[i] for i in second])
    got = _triples(api.align_pairs(ctx, seqs, first, second))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def test_the_carry_column_on_either_side_of_the_lds_limit(ctx):
    """Two stripes and a second sequence long enough that the carry column fills a workgroup's LDS (700 x 6 300: 158 420 of 163 840 bytes) or no
    longer fits it (257 x 6 600 goes to global memory); the fixture's own long pairs lie far from that limit"""
    t = synth.template(91, 0, 6600)
    long_one = synth.to_ascii(synth.member(91, 0, 0, t))
    seqs = [synth.to_ascii(t[3000:3700]), long_one[:6300], synth.to_ascii(t[100:357]), (long_one + long_one)[:6600], synth.to_ascii(t[:300]), long_one[:5000]]
    first, second = [0, 2, 4, 2], [1, 3, 5, 1]
    for params in ((1, -1, 2, 1), (2, -3, 5, 2)):
        want = align_util.align_many([seqs[i] for i in first], [seqs[i] for i in second], params, step=4096)
        got = _triples(api.align_pairs(ctx, seqs, first, second, *params))
        assert np.array_equal(got, want), (params, got.tolist(), want.tolist())
    assert ctx.last_kernel_info()[0] == "k_align_pairs<carry in global memory>"
    api.align_pairs(ctx, seqs, first[:1], second[:1])
    assert ctx.last_kernel_info()[0] == "k_align_pairs<carry in LDS>"


def test_an_empty_list_and_the_refusals(ctx, fx):
    r = api.align_pairs(ctx, fx.seqs, [], [])
    assert r["score"].size == 0 and r["identity"].size == 0
    assert api.align_pairs(ctx, [], [], [])["length"].size == 0

    def refused(seqs, first, second, *params):
        out = tuple(np.full(len(first), -7, dtype=np.int32) for _ in range(3))
        with pytest.raises(api.MscError) as e:
            api.align_pairs(ctx, seqs, first, second, *params, out=out)
        assert e.value.code == -1, e.value          # MSC_ERR_INVALID_ARG
        assert all((o == -7).all() for o in out), "a refused call wrote an output"

    ok = [b"ACGT", b"AC"]
    refused(ok + [b""], [0, 2], [1, 1])                       # a length of 0
    refused(ok + [b"A" * 32768], [0, 0], [1, 2])              # a length of 32 768
    refused(ok, [0, 1], [1, 2])                               # an index past n_seqs
    for at in range(4):                                       # a parameter of 101 (and of -101)
        for v in (101, -101):
            params = [1, -1, 2, 1]
            params[at] = v
            refused(ok, [0, 1], [1, 0], *params)
    # an unlisted sequence may be anything; the limits themselves are legal
    r = api.align_pairs(ctx, ok + [b"", b"A" * 32768], [0], [1], 100, -100, 100, 100)
    assert _triples(r).tolist() == [list(align_util.align(ok[0], ok[1], (100, -100, 100, 100)))]


def _fastcar(tmp_path, weights, extra, prefix):
    exe = os.path.join(ROOT, "meshclust2_amd", "host", "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "meshclust2_amd", "host")])
    r = subprocess.run([exe, "db.fa", "--query", "q.fa", "--recover", os.path.join(GOLDEN, weights), "--output", prefix] + extra, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-2000:]
    return open(str(tmp_path / (prefix + "0")), "rb").read(), r.stderr.decode()


def test_fastcar_align_adds_the_alignment_identity_of_every_line(tmp_path):
    """the inputs of tests/golden/fastcar_k5_u16.out (test_fastcar_k5_u16_fixture_route, tests/test_gpu_qxm_direct.py)"""
    db, h = synth.families(41, 300, 1000, family=10, length_jitter=150)
    q, hq = synth.families(41, 40, 1000, family=10, length_jitter=150)
    q = [x[:len(x) - 7] for x in q]
    synth.write_fasta(str(tmp_path / "db.fa"), db, h)
    synth.write_fasta(str(tmp_path / "q.fa"), q, [x.replace(">seq", ">qry") for x in hq])
    exp = open(os.path.join(GOLDEN, "fastcar_k5_u16.out"), "rb").read()
    plain, _ = _fastcar(tmp_path, "weights_k5_u16.txt", [], "plain")
    assert plain == exp, "without --align the output is the committed one, byte for byte"
    got, err = _fastcar(tmp_path, "weights_k5_u16.txt", ["--align", "--kernels"], "aligned")
    assert "kernel: k_align_pairs<" in err, err
    lines, exp_lines = got.decode().splitlines(), exp.decode().splitlines()
    assert len(lines) == len(exp_lines) > 100
    qs, ds, cols = [], [], []
    for ln, e in zip(lines, exp_lines):
        head, col = ln.rsplit("\t", 1)
        assert head == e, (ln, e)
        a, b = head.split("\t")[:2]
        qs.append(q[int(a.strip()[3:])])
        ds.append(db[int(b.strip()[3:])])
        cols.append(col)
    want = align_util.align_many(qs, ds, step=128)
    assert cols == ["%g" % (100 * (m / ln)) for _, ln, m in want.tolist()]          # the format of the identity column: the stream's default


def test_fastcar_align_on_both_strands_aligns_the_reversed_query(tmp_path):
    kw = dict(family=4, length_jitter=120, sub_rate=0.01, indel_rate=0.002)          # (close enough for the model of weights_k9_u32_fc.txt to call them)
    db, h = synth.families(43, 24, 1000, **kw)
    q, hq = synth.families(43, 8, 1000, **kw)
    q = [x[:len(x) - 5] for x in q]
    q = [x[::-1].translate(_COMP) if i % 2 else x for i, x in enumerate(q)]          # every odd read is the other strand
    synth.write_fasta(str(tmp_path / "db.fa"), db, h)
    synth.write_fasta(str(tmp_path / "q.fa"), q, [x.replace(">seq", ">qry") for x in hq])
    plain, _ = _fastcar(tmp_path, "weights_k9_u32_fc.txt", ["--both-strands"], "plain")
    got, _ = _fastcar(tmp_path, "weights_k9_u32_fc.txt", ["--both-strands", "--align"], "aligned")
    lines, plain_lines = got.decode().splitlines(), plain.decode().splitlines()
    assert len(lines) == len(plain_lines) > 8
    qs, ds, cols, strands = [], [], [], []
    for ln, e in zip(lines, plain_lines):
        head, col = ln.rsplit("\t", 1)
        assert head == e, (ln, e)
        a, b, _, strand = head.split("\t")
        qi = int(a.strip()[3:])
        qs.append(q[qi][::-1].translate(_COMP) if strand == "-" else q[qi])
        ds.append(db[int(b.strip()[3:])])
        cols.append(col)
        strands.append(strand)
    assert "-" in strands and "+" in strands
    want = align_util.align_many(qs, ds, step=128)
    assert cols == ["%g" % (100 * (m / ln)) for _, ln, m in want.tolist()]
    # a `-` hit aligned as given would be far from it: the column is the reversed query's
    k = strands.index("-")
    as_given = align_util.align(qs[k][::-1].translate(_COMP), ds[k])
    assert as_given[2] / as_given[1] < 0.7 < want[k][2] / want[k][1]
