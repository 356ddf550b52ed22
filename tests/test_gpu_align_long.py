"""msc_align_pairs_long, msc_align_pairs_long_banded and msc_align_pairs_long_auto on the device, and msc_fastcar --align on a 40 kb sequence
(DESIGN.md 4.6g).

k_align_tiles is held (1) to the kernels of the short entries, bit for bit, on every pair those can run -- MSC_ALIGN_LONG_ALL=1 sends short
pairs through the tiles, at tile heights that cut them into many -- and (2) to the reference's own integers on pairs past 32 767 bytes
(tests/golden/align_long.npz, written by tests/golden/gen_align_long_golden.py)."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import align_util
from meshclust2_amd import api, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NO_BAND = 0xffffffff
BANDS = [1, 17, 64, 300]
DEFAULT_ROWS = 256          # kAlignTileRows (csrc/msc_align_long.h)


@contextlib.contextmanager
def switches(long_all=None, tile_rows=None):
    """the library reads both on every call"""
    keep = {k: os.environ.get(k) for k in ("MSC_ALIGN_LONG_ALL", "MSC_ALIGN_TILE_ROWS")}
    for k, v in (("MSC_ALIGN_LONG_ALL", long_all), ("MSC_ALIGN_TILE_ROWS", tile_rows)):
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return align_util.Fixture()


class LongFixture(align_util.Fixture):
    def __init__(self):
        path = os.path.join(GOLDEN, "align_long.npz")
        super().__init__(path)
        z = np.load(path)
        self.have = z["have"]
        self.named = dict(zip(z["names"].tolist(), z["named"].tolist()))


@pytest.fixture(scope="module")
def lfx():
    return LongFixture()


@pytest.fixture(scope="module")
def short_pairs(fx):
    """the fixture's 201 pairs and 1 000 seeded ones of 1 .. 1 500 bytes, half of them related -> seqs, first, second"""
    rs = np.random.RandomState(20261)
    seqs = list(fx.seqs)
    first, second = fx.first.tolist(), fx.second.tolist()
    for p in range(1000):
        la, lb = int(rs.randint(1, 1501)), int(rs.randint(1, 1501))
        a = synth.template(700 + p, 0, la)
        if p % 2:
            b = synth.member(700 + p, 0, 0, synth.template(700 + p, 0, max(la, lb)))[:lb]          # a mutated copy that starts where a starts
        else:
            b = synth.template(700 + p, 1, lb)
        if b.size == 0:
            b = a[:1]
        seqs += [synth.to_ascii(a), synth.to_ascii(b)]
        first.append(len(seqs) - 2)
        second.append(len(seqs) - 1)
    return seqs, np.array(first, dtype=np.uint32), np.array(second, dtype=np.uint32)


@pytest.fixture(scope="module")
def short_oracle(ctx, short_pairs):
    """what the kernels of the short entries give for short_pairs: computed once, never changed"""
    seqs, first, second = short_pairs
    with switches():
        full = _triples(api.align_pairs(ctx, seqs, first, second))
        banded = {w: _quad(api.align_pairs_banded(ctx, seqs, first, second, w)) for w in BANDS}
    full.setflags(write=False)
    for v in banded.values():
        v.setflags(write=False)
    return full, banded


def _triples(r):
    return np.stack([r["score"], r["length"], r["matches"]], axis=1).astype(np.int64)


def _quad(r):
    return np.stack([r["score"], r["length"], r["matches"], r["certified"]], axis=1).astype(np.int64)


def _same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def _tiles(ctx, rows):
    assert ctx.last_kernel_info()[0] == "k_align_tiles<wide states, %d rows a tile>" % rows, ctx.last_kernel_info()


@pytest.mark.parametrize("rows", [64, 100])
def test_the_tiles_are_the_short_kernels_bit_for_bit(ctx, short_pairs, short_oracle, rows):
    seqs, first, second = short_pairs
    full, banded = short_oracle
    assert first.size == 1201
    with switches(long_all=1, tile_rows=rows):
        _same(_triples(api.align_pairs_long(ctx, seqs, first, second)), full, ("full grid", rows))
        _tiles(ctx, rows)
        for w in BANDS:
            got = _quad(api.align_pairs_long_banded(ctx, seqs, first, second, w))
            _tiles(ctx, rows)
            _same(got, banded[w], ("half-width", w, rows))
            assert 0 < got[:, 3].sum() < first.size or w == 300          # (uncertified pairs are compared too: the band defines them)
    # without the switch the same call runs the short kernels
    with switches(tile_rows=rows):
        _same(_triples(api.align_pairs_long(ctx, seqs, first, second)), full, "routed")
        assert ctx.last_kernel_info()[0].startswith("k_align_pairs<"), ctx.last_kernel_info()
        _same(_quad(api.align_pairs_long_banded(ctx, seqs, first, second, 17)), banded[17], "routed, banded")
        assert ctx.last_kernel_info()[0].startswith("k_align_band<"), ctx.last_kernel_info()


def test_the_edges_of_stripes_and_row_blocks(ctx):
    las, lbs = [255, 256, 257, 512, 513], [63, 64, 65, 127, 128, 129]
    fam = synth.template(91, 0, 600)
    seqs, first, second = [], [], []
    for la in las:
        for lb in lbs:
            seqs += [synth.to_ascii(fam[:la]), synth.to_ascii(synth.member(91, 0, la * 1000 + lb, fam)[:lb])]
            first += [len(seqs) - 2, len(seqs) - 1]          # both orders
            second += [len(seqs) - 1, len(seqs) - 2]
    with switches():
        full = _triples(api.align_pairs(ctx, seqs, first, second))
        banded = _quad(api.align_pairs_banded(ctx, seqs, first, second, 8))
    with switches(long_all=1, tile_rows=64):
        _same(_triples(api.align_pairs_long(ctx, seqs, first, second)), full, "full grid")
        _tiles(ctx, 64)
        _same(_quad(api.align_pairs_long_banded(ctx, seqs, first, second, 8)), banded, "half-width 8")
        _tiles(ctx, 64)


def test_the_long_fixture_is_the_references(ctx, lfx):
    for s, params in enumerate(lfx.params):
        sel = np.nonzero(lfx.have[s])[0]
        with switches():
            r = api.align_pairs_long(ctx, lfx.seqs, lfx.first[sel], lfx.second[sel], *[int(v) for v in params])
        _tiles(ctx, DEFAULT_ROWS)
        _same(_triples(r), lfx.result[s][sel].astype(np.int64), params.tolist())
    assert lfx.result[0][lfx.named["similar"], 2] > 65535 and lfx.result[0][lfx.named["homopolymer"], 2] > 65535
    p = lfx.named["many_tiles"]
    with switches(tile_rows=512):
        r = api.align_pairs_long(ctx, lfx.seqs, lfx.first[p:p + 1], lfx.second[p:p + 1])
    _tiles(ctx, 512)
    _same(_triples(r), lfx.result[0][p:p + 1].astype(np.int64), "512 rows a tile")


def test_auto_on_the_long_fixture_and_a_mixed_list(ctx, lfx, fx):
    sel = np.nonzero(lfx.have[0])[0]
    with switches():
        r = api.align_pairs_long_auto(ctx, lfx.seqs, lfx.first[sel], lfx.second[sel])
    _same(_triples(r), lfx.result[0][sel].astype(np.int64), "auto")
    used = dict(zip(sel.tolist(), r["band_used"].tolist()))
    assert used[lfx.named["similar"]] <= 1024, used
    assert used[lfx.named["unrelated"]] == NO_BAND and used[lfx.named["unrelated"] + 1] == NO_BAND, used
    # short and long pairs in one list, interleaved: the caller's order
    short = np.nonzero(fx.cells() <= 300 * 300)[0][:40]
    seqs = list(fx.seqs) + list(lfx.seqs)
    thin = np.arange(4)
    first = np.concatenate([fx.first[short[:20]], lfx.first[thin[:2]] + len(fx.seqs), fx.first[short[20:]], lfx.first[thin[2:]] + len(fx.seqs)]).astype(np.uint32)
    second = np.concatenate([fx.second[short[:20]], lfx.second[thin[:2]] + len(fx.seqs), fx.second[short[20:]], lfx.second[thin[2:]] + len(fx.seqs)]).astype(np.uint32)
    want = np.concatenate([fx.result[0][short[:20]], lfx.result[0][thin[:2]], fx.result[0][short[20:]], lfx.result[0][thin[2:]]]).astype(np.int64)
    with switches():
        _same(_triples(api.align_pairs_long_auto(ctx, seqs, first, second)), want, "mixed, auto")
        _same(_triples(api.align_pairs_long(ctx, seqs, first, second)), want, "mixed")
        _tiles(ctx, DEFAULT_ROWS)


def test_a_banded_call_after_a_full_one_reads_nothing_stale():
    """a context of its own: the first call leaves its borders in the scratch buffer, the second reuses the buffer at a narrow band"""
    c = api.Context(0)
    try:
        t = synth.template(93, 0, 3000)
        with switches(long_all=1, tile_rows=64):
            api.align_pairs_long(c, [synth.to_ascii(t), synth.to_ascii(synth.member(93, 0, 0, t))], [0], [1])
        seqs, first, second = [], [], []
        for k in range(6):
            u = synth.template(95 + k, 0, 2900 + 37 * k)
            seqs += [synth.to_ascii(u), synth.to_ascii(synth.member(95 + k, 0, 0, u) if k % 2 else synth.template(95 + k, 1, 3000 - 41 * k))]
            first.append(2 * k)
            second.append(2 * k + 1)
        with switches():
            want = _quad(api.align_pairs_banded(c, seqs, first, second, 8))
        with switches(long_all=1, tile_rows=64):
            got = _quad(api.align_pairs_long_banded(c, seqs, first, second, 8))
        assert c.last_kernel_info()[0].startswith("k_align_tiles<")
        _same(got, want, "half-width 8 over a used scratch buffer")
    finally:
        c.close()


def test_an_empty_list_and_the_refusals(ctx):
    calls = ((api.align_pairs_long, None, {}), (api.align_pairs_long_banded, np.uint8, dict(band=4)), (api.align_pairs_long_auto, np.uint32, dict(first_band=4)))
    for call, last, kw in calls:
        assert call(ctx, [b"ACGT"], [], [], **kw)["score"].size == 0
        assert call(ctx, [], [], [], **kw)["length"].size == 0

        def refused(seqs, first, second, params=(1, -1, 2, 1)):
            out = tuple(np.full(len(first), -7, dtype=np.int32) for _ in range(3)) + ((np.full(len(first), 9, dtype=last),) if last else ())
            with pytest.raises(api.MscError) as e:
                call(ctx, seqs, first, second, out=out, match=params[0], mismatch=params[1], gap_open=params[2], gap_continue=params[3], **kw)
            assert e.value.code == -1, e.value          # MSC_ERR_INVALID_ARG
            assert all((o == -7).all() for o in out[:3]) and all((o == 9).all() for o in out[3:]), "a refused call wrote an output"

        ok = [b"ACGT", b"AC"]
        refused(ok + [b""], [0, 2], [1, 1])                       # a length of 0
        refused(ok + [b"A" * 1048576], [0, 0], [1, 2])            # a length of 1 048 576
        refused(ok, [0, 1], [1, 2])                               # an index past n_seqs
        params = [1, -1, 2, 101]
        refused(ok, [0, 1], [1, 0], params)                       # a parameter of 101
    # the short entries keep their limit
    with pytest.raises(api.MscError):
        api.align_pairs(ctx, [b"A" * 32768, b"AC"], [0], [1])


def test_the_short_entries_ignore_the_switches(ctx):
    """the short entries share the driver of the _long ones with the tile route shut: the two switches must not reach them"""
    lens = [(1, 1), (1, 600), (600, 1), (63, 64), (255, 300), (256, 256), (256, 17), (257, 257), (257, 599), (511, 130), (513, 40), (600, 600), (300, 256)]
    seqs, first, second = [], [], []
    for k, (la, lb) in enumerate(lens):
        t = synth.template(301 + k, 0, 700)
        seqs += [synth.to_ascii(t[:la]), synth.to_ascii((synth.member(301 + k, 0, 0, t) if k % 3 else synth.template(301 + k, 1, 600))[:lb])]
        first.append(2 * k)
        second.append(2 * k + 1)
    assert all(len(seqs[2 * k]) == la and len(seqs[2 * k + 1]) == lb for k, (la, lb) in enumerate(lens))
    calls = ((api.align_pairs, {}, "k_align_pairs<"), (api.align_pairs_banded, dict(band=17), "k_align_band<"), (api.align_pairs_auto, {}, None))
    with switches():
        want = [call(ctx, seqs, first, second, **kw) for call, kw, _ in calls]
        auto_kernel = ctx.last_kernel_info()[0]
    assert auto_kernel.startswith("k_align_band<") or auto_kernel.startswith("k_align_pairs<"), auto_kernel
    with switches(long_all=1, tile_rows=16):
        for (call, kw, kernel), w in zip(calls, want):
            got = call(ctx, seqs, first, second, **kw)
            name = ctx.last_kernel_info()[0]
            assert name.startswith("k_align_pairs<") or name.startswith("k_align_band<"), (call.__name__, name)
            assert name == auto_kernel if kernel is None else name.startswith(kernel), (call.__name__, name)
            assert sorted(got) == sorted(w)
            for key in w:
                assert np.array_equal(got[key], w[key]), (call.__name__, key, got[key].tolist(), w[key].tolist())
        # and they keep their limit: a 32 768-byte sequence is refused by name
        for call, kw, _ in calls:
            with pytest.raises(api.MscError) as e:
                call(ctx, [b"A" * 32768, b"AC"], [0], [1], **kw)
            assert e.value.code == -1, e.value          # MSC_ERR_INVALID_ARG
            assert call.__name__.replace("align", "msc_align") in str(e.value) and "32767" in str(e.value), str(e.value)


def test_fastcar_align_reports_a_40_kb_hit(tmp_path, ctx):
    db, h = synth.families(41, 30, 1000, family=10, length_jitter=150)
    q, hq = synth.families(41, 4, 1000, family=10, length_jitter=150)
    t = synth.template(97, 0, 40000)
    db.append(synth.to_ascii(t))
    h.append(">seq%d template_99" % (len(db) - 1))
    q.append(synth.to_ascii(synth.member(97, 0, 0, t, sub_rate=0.01, indel_rate=0.002)))
    hq.append(">seq%d template_99" % (len(q) - 1))
    synth.write_fasta(str(tmp_path / "db.fa"), db, h)
    synth.write_fasta(str(tmp_path / "q.fa"), q, [x.replace(">seq", ">qry") for x in hq])
    exe = os.path.join(ROOT, "meshclust2_amd", "host", "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "meshclust2_amd", "host")])
    outs = []
    for prefix, extra in (("plain", ["--align"]), ("banded", ["--align", "--align-band", "0"])):
        r = subprocess.run([exe, "db.fa", "--query", "q.fa", "--recover", os.path.join(GOLDEN, "weights_k5_u16.txt"), "--output", prefix] + extra, cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-2000:]
        outs.append(open(str(tmp_path / (prefix + "0")), "rb").read())
    assert outs[0] == outs[1]
    qs, ds, cols = [], [], []
    for ln in outs[0].decode().splitlines():
        head, col = ln.rsplit("\t", 1)
        a, b = head.split("\t")[:2]
        qs.append(q[int(a.strip()[3:])])
        ds.append(db[int(b.strip()[3:])])
        cols.append(col)
    assert any(len(x) > 32767 and len(y) > 32767 for x, y in zip(qs, ds)), "the 40 kb hit is not among the reported pairs"
    seqs = qs + ds
    with switches():
        r = api.align_pairs_long(ctx, seqs, np.arange(len(qs)), np.arange(len(qs)) + len(qs))
    assert cols == ["%g" % (100 * v) for v in r["identity"].tolist()]
