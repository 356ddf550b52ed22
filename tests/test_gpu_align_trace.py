"""msc_align_pairs_trace on the device, and msc_fastcar --align --cigar.

The triples are held to the reference's own integers (tests/golden/align_pairs.npz), the runs to tests/golden/align_trace.npz (every fixture
pair) and, byte for byte, to tests/align_trace_util.py, the numpy restatement of DESIGN.md 4.6h that tests/test_align_trace_cpu.py holds to
the same fixtures; pairs too long for the restatement are held to the section's invariants through align_trace_util.replay."""
import os
import subprocess

import numpy as np
import pytest

import align_trace_util
import align_util
from meshclust2_amd import api, synth
from align_trace_util import EDGE_LA, EDGE_LB, SMALL, edge_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return align_util.Fixture()


def _raw(s):
    return s if isinstance(s, bytes) else s.encode()


def _triples(r):
    return np.stack([r["score"], r["length"], r["matches"]], axis=1)


def _runs(r, p):
    return r["ops"][int(r["op_offsets"][p]):int(r["op_offsets"][p + 1])]


def _is_the_restatements(ctx, firsts, seconds, params):
    """one call over the pairs (firsts[p], seconds[p]): triples and runs equal the restatement's, byte for byte; -> (result, real flags)"""
    seqs = list(firsts) + list(seconds)
    n = len(firsts)
    r = api.align_pairs_trace(ctx, seqs, np.arange(n), np.arange(n) + n, *params)
    triples, ops, real = align_trace_util.trace_many(firsts, seconds, params)
    assert np.array_equal(_triples(r), triples), params
    assert r["op_offsets"].dtype == np.uint64 and r["ops"].dtype == np.uint32
    assert r["op_offsets"][0] == 0 and r["op_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(o) for o in ops])]).tolist(), params
    for p in range(n):
        assert _runs(r, p).tobytes() == np.asarray(ops[p], dtype=np.uint32).tobytes(), (params, p, api.cigar_string(_runs(r, p)), align_trace_util.cigar_string(ops[p]))
    return r, real


def test_every_fixture_pair_under_every_parameter_set(ctx, fx):
    gold = align_trace_util.Fixture()
    small = fx.cells() <= SMALL
    for s, params in enumerate(fx.params):
        r = api.align_pairs_trace(ctx, fx.seqs, fx.first, fx.second, *[int(v) for v in params])
        got = _triples(r)
        bad = np.nonzero((got != fx.result[s]).any(axis=1))[0]
        assert bad.size == 0, (params.tolist(), int(bad[0]), got[bad[0]].tolist(), fx.result[s][bad[0]].tolist())
        assert np.array_equal(r["identity"], fx.result[s][:, 2] / fx.result[s][:, 1].astype(np.float64))
        off = r["op_offsets"]
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 1).all() and int(off[-1]) == r["ops"].size
        assert np.diff(off.astype(np.int64)).tolist() == gold.runs[s].tolist()
        for p in range(fx.first.size):
            runs = _runs(r, p)
            assert align_trace_util.digest(runs) == gold.sha256[s][p].tobytes(), (params.tolist(), p)
            score, columns, same = align_trace_util.replay(runs, fx.seqs[fx.first[p]], fx.seqs[fx.second[p]], params)
            assert columns == got[p, 1] and (params[0] == params[1] or same == got[p, 2]), (params.tolist(), p)
            assert not gold.real[s][p] or score == got[p, 0], (params.tolist(), p)
        assert gold.real[s][small].all(), "the three sets' small pairs are all real"
    name, per_read = ctx.last_kernel_info()
    assert name.startswith("k_align_pairs_dirs<") and per_read == 0, name


def test_the_edges_are_the_restatements_byte_for_byte(ctx):
    firsts, seconds = edge_pairs()
    assert {(len(a), len(b)) for a, b in zip(firsts, seconds)} == {(a, b) for a in EDGE_LA for b in EDGE_LB}
    for params in ((1, -1, 2, 1), (2, -3, 5, 2)):
        _is_the_restatements(ctx, firsts, seconds, params)


def test_a_sequence_against_itself_and_against_its_ends(ctx):
    rs = np.random.RandomState(3)
    whole = LETTERS[rs.randint(0, 4, 400)].copy()
    whole[0] = ord("A") if whole[100] != ord("A") else ord("C")          # (no equally good alignment with the gap a column further in)
    whole[399] = ord("A") if whole[299] != ord("A") else ord("C")
    whole = whole.tobytes()
    r = api.align_pairs_trace(ctx, [whole], [0], [0])
    assert api.cigar_string(r["ops"]) == "400=" and r["op_offsets"].tolist() == [0, 1]
    # a suffix of the other sequence: the bytes it lacks lead the alignment; a prefix: they trail it
    firsts, seconds = [whole[100:], whole, whole[:300], whole], [whole, whole[100:], whole, whole[:300]]
    r, real = _is_the_restatements(ctx, firsts, seconds, (1, -1, 2, 1))
    assert real.all()
    assert [api.cigar_string(_runs(r, p)) for p in range(4)] == ["100D300=", "100I300=", "300=100D", "300=100I"]


def test_paths_that_are_not_real_keep_both_counts(ctx):
    rs = np.random.RandomState(11)
    firsts = [LETTERS[rs.randint(0, 4, int(rs.randint(1, 121)))].tobytes() for _ in range(120)]
    seconds = [LETTERS[rs.randint(0, 4, int(rs.randint(1, 121)))].tobytes() for _ in range(120)]
    unreal = 0
    for params in ((1, 1, 0, 0), (0, 0, 1, 1)):
        r, real = _is_the_restatements(ctx, firsts, seconds, params)
        unreal += int((~real).sum())
        for p in range(len(firsts)):
            _, columns, _ = align_trace_util.replay(_runs(r, p), firsts[p], seconds[p], params)
            assert columns == r["length"][p]
    assert unreal > 0


def test_repeated_pairs_the_list_reversed_and_two_calls(ctx, fx):
    sel = np.nonzero(fx.cells() <= SMALL)[0]
    first, second = fx.first[sel], fx.second[sel]
    base = api.align_pairs_trace(ctx, fx.seqs, first, second)
    per_pair = [_runs(base, p).tobytes() for p in range(sel.size)]
    order = np.repeat(np.arange(sel.size)[::-1], 2)
    r = api.align_pairs_trace(ctx, fx.seqs, first[order], second[order])
    assert np.array_equal(_triples(r), _triples(base)[order])
    assert [_runs(r, p).tobytes() for p in range(order.size)] == [per_pair[k] for k in order]
    again = api.align_pairs_trace(ctx, fx.seqs, first[order], second[order])
    assert again["ops"].tobytes() == r["ops"].tobytes() and again["op_offsets"].tobytes() == r["op_offsets"].tobytes()
    assert _triples(again).tobytes() == _triples(r).tobytes()


def test_the_carry_column_on_either_side_of_the_lds_limit(ctx):
    """the pairs of test_gpu_align.py's carry test: 700 x 6 300 fills a workgroup's LDS, 257 x 6 600 keeps its carry in global memory"""
    t = synth.template(91, 0, 6600)
    long_one = synth.to_ascii(synth.member(91, 0, 0, t))
    seqs = [synth.to_ascii(t[3000:3700]), long_one[:6300], synth.to_ascii(t[100:357]), (long_one + long_one)[:6600], synth.to_ascii(t[:300]), long_one[:5000]]
    first, second = [0, 2, 4, 2], [1, 3, 5, 1]
    raw = [_raw(s) for s in seqs]
    for params in ((1, -1, 2, 1), (2, -3, 5, 2)):
        want = align_util.align_many([seqs[i] for i in first], [seqs[i] for i in second], params, step=4096)
        r = api.align_pairs_trace(ctx, seqs, first, second, *params)
        assert np.array_equal(_triples(r), want), (params, _triples(r).tolist(), want.tolist())
        for p in range(len(first)):
            assert align_trace_util.replay(_runs(r, p), raw[first[p]], raw[second[p]], params) == tuple(want[p]), (params, p)
    assert ctx.last_kernel_info()[0] == "k_align_pairs_dirs<carry in global memory>"
    api.align_pairs_trace(ctx, seqs, first[:1], second[:1])
    assert ctx.last_kernel_info()[0] == "k_align_pairs_dirs<carry in LDS>"


def test_groups_do_not_show_in_the_result(ctx, monkeypatch):
    rs = np.random.RandomState(20)
    seqs = [LETTERS[rs.randint(0, 4, int(rs.randint(80, 301)))].tobytes() for _ in range(200)]
    for i in range(1, 200, 2):          # every other one a mutated copy of its neighbour
        src = np.frombuffer(seqs[i - 1], dtype=np.uint8).copy()
        hit = rs.rand(src.size) < 0.08
        src[hit] = LETTERS[rs.randint(0, 4, int(hit.sum()))]
        seqs[i] = np.delete(src, rs.randint(0, src.size, 3)).tobytes() + b"ACGT"
    first = rs.randint(0, 200, 600).astype(np.uint32)
    second = (first ^ (rs.rand(600) < 0.7)).astype(np.uint32)          # mostly the related neighbour
    ln = np.array([len(s) for s in seqs])
    need = (((ln[first] + 255) // 256) * (ln[second] + 63) * 128).sum()
    assert need > 8 << 20          # several groups of 1 MiB
    whole = api.align_pairs_trace(ctx, seqs, first, second)
    monkeypatch.setenv("MSC_ALIGN_TRACE_BYTES", str(1 << 20))
    dealt = api.align_pairs_trace(ctx, seqs, first, second)
    for key in ("score", "length", "matches", "op_offsets", "ops"):
        assert dealt[key].tobytes() == whole[key].tobytes(), key
    # a pair above the cap is a group of its own and still runs
    monkeypatch.setenv("MSC_ALIGN_TRACE_BYTES", "4096")
    few = api.align_pairs_trace(ctx, seqs, first[:40], second[:40])
    assert few["ops"].tobytes() == whole["ops"][:int(whole["op_offsets"][40])].tobytes() and np.array_equal(few["op_offsets"], whole["op_offsets"][:41])


def test_fetch_in_pieces_and_the_refusals(ctx, fx):
    sel = np.nonzero(fx.cells() <= SMALL)[0][:60]
    r = api.align_pairs_trace(ctx, fx.seqs, fx.first[sel], fx.second[sel])
    total = int(r["op_offsets"][-1])
    pieces = [api.align_trace_fetch(ctx, at, min(7, total - at)) for at in range(0, total, 7)]
    assert np.concatenate(pieces).tobytes() == r["ops"].tobytes()
    p = 17
    assert api.align_trace_fetch(ctx, int(r["op_offsets"][p]), int(r["op_offsets"][p + 1] - r["op_offsets"][p])).tobytes() == _runs(r, p).tobytes()
    assert api.align_trace_fetch(ctx, total, 0).size == 0
    for at, n in ((0, total + 1), (total, 1), (total + 1, 0)):
        with pytest.raises(api.MscError) as e:
            api.align_trace_fetch(ctx, at, n)
        assert e.value.code == -1, e.value          # MSC_ERR_INVALID_ARG

    def refused(seqs, first, second, *params):
        out = tuple(np.full(len(first), -7, dtype=np.int32) for _ in range(3)) + (np.full(len(first) + 1, 99, dtype=np.uint64),)
        with pytest.raises(api.MscError) as e:
            api.align_pairs_trace(ctx, seqs, first, second, *params, out=out)
        assert e.value.code == -1, e.value
        assert all((o == -7).all() for o in out[:3]) and (out[3] == 99).all(), "a refused call wrote an output"

    ok = [b"ACGT", b"AC"]
    refused(ok + [b""], [0, 2], [1, 1])                       # a length of 0
    refused(ok + [b"A" * 32768], [0, 0], [1, 2])              # a length of 32 768
    refused(ok, [0, 1], [1, 2])                               # an index past n_seqs
    refused(ok, [0, 1], [1, 0], 1, -1, 101, 1)                # a parameter of 101
    # a refused call leaves the list of the call before in place
    assert api.align_trace_fetch(ctx, 0, total).tobytes() == r["ops"].tobytes()
    empty = api.align_pairs_trace(ctx, fx.seqs, [], [])
    assert empty["op_offsets"].tolist() == [0] and empty["ops"].size == 0 and empty["score"].size == 0


def _fastcar(tmp_path, extra, prefix, ok=True):
    exe = os.path.join(ROOT, "meshclust2_amd", "host", "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "meshclust2_amd", "host")])
    r = subprocess.run([exe, "db.fa", "--query", "q.fa", "--recover", os.path.join(GOLDEN, "weights_k5_u16.txt"), "--output", prefix] + extra, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    if not ok:
        return r
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-2000:]
    return open(str(tmp_path / (prefix + "0")), "rb").read(), r.stderr.decode()


def test_fastcar_cigar_adds_the_hits_cigar_as_the_last_column(tmp_path):
    """the inputs of tests/golden/fastcar_k5_u16.out (test_gpu_align.py's driver test)"""
    db, h = synth.families(41, 300, 1000, family=10, length_jitter=150)
    q, hq = synth.families(41, 40, 1000, family=10, length_jitter=150)
    q = [x[:len(x) - 7] for x in q]
    synth.write_fasta(str(tmp_path / "db.fa"), db, h)
    synth.write_fasta(str(tmp_path / "q.fa"), q, [x.replace(">seq", ">qry") for x in hq])
    # refused before a device is opened: nothing on stdout, no output file
    for extra in (["--cigar"], ["--align", "--align-band", "16", "--cigar"]):
        r = _fastcar(tmp_path, extra, "refused", ok=False)
        assert r.returncode != 0 and b"--cigar" in r.stderr and not os.path.exists(str(tmp_path / "refused0")), (r.stdout + r.stderr).decode()
    exp = open(os.path.join(GOLDEN, "fastcar_k5_u16.out"), "rb").read()
    plain, _ = _fastcar(tmp_path, [], "plain")
    assert plain == exp
    aligned, _ = _fastcar(tmp_path, ["--align"], "aligned")
    lines = aligned.decode().splitlines()
    assert [ln.rsplit("\t", 1)[0] for ln in lines] == exp.decode().splitlines()          # with --align alone: today's bytes (test_gpu_align.py holds the column)
    got, err = _fastcar(tmp_path, ["--align", "--cigar", "--kernels"], "traced")
    assert "kernel: k_align_pairs_dirs<" in err, err
    traced = got.decode().splitlines()
    assert len(traced) == len(lines) > 100
    qs, ds, cols = [], [], []
    for ln, e in zip(traced, lines):
        head, col = ln.rsplit("\t", 1)
        assert head == e, (ln, e)
        a, b = head.split("\t")[:2]
        qs.append(_raw(q[int(a.strip()[3:])]))
        ds.append(_raw(db[int(b.strip()[3:])]))
        cols.append(col)
    _, ops, _ = align_trace_util.trace_many(qs, ds, step=128)
    assert cols == [api.cigar_string(o) for o in ops]
