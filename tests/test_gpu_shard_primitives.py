"""The per-GPU primitives of the sharded driver (meshclust2_amd/host/msc_sharded.hpp over msc_gpu_engine.hpp) held to the CPU oracle and
to the single-GPU entry points, with N <= 4 ranks emulated in one process: one Context per rank, the collectives done on the host the
way msc_sharded.hpp::column_sums does them (dense: the ranks' uint64 payloads added word by word; sparse: the payloads gathered, each
padded to the largest rounded up to 16), the result copied into a device buffer of every rank.

  msc_colsum_partial / msc_colsum_nearest   every rank's nearest member of each list, its distance and the list's size over all ranks
  msc_hist_pack / unpack / set_reset         a slot as one byte range: exact copies that score as their source, stale mirrors, errors
  msc_filter_batch                           Trainer::filter of many centres in one pass
"""
import ctypes as C

import numpy as np
import pytest

from golden_util import cfg4_sequences, weights_text
from meshclust2_amd import api, synth
from meshclust2_amd._capi import MscError

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_OOM = -1, -4
ALL_MASK = api.FEAT_SLOW


def up16(v):
    return (v + 15) & ~15


@pytest.fixture(scope="module")
def ranks():
    cs = [api.Context(0) for _ in range(4)]
    yield cs
    for c in cs:
        c.close()


# ------------------------------------------------------------------------------------------------ points
def _pool():
    """25 sequences: two families of relatives (0-11), mixed lengths 200 b - 5 kb (12-15), three copies of sequence 0 (16-18: with it,
    four identical members whose distances tie exactly), five whose k-mer counts pass 255 (19-23: u8 bins saturate), one shorter than k"""
    fam, _ = synth.families(9101, 12, 1500, family=6)
    mixed = [synth.families(9102 + i, 1, ln, family=1)[0][0] for i, ln in enumerate((200, 700, 2300, 5000))]
    sat = [b"A" * 900 + fam[1][:300], b"ACGT" * 400, b"AC" * 400 + b"G" * 500, b"T" * 600 + fam[2][:800], b"CCA" * 350]
    return list(fam) + mixed + [fam[0]] * 3 + sat + [b"ACG"]


POOL = _pool()
TWINS = [0, 16, 17, 18]
SAT = [19, 20, 21, 22, 23]
# lists over POOL: empty, one member, many, exact ties, saturated bins, mixed lengths and a member shorter than k
LISTS_A = [[], [3], list(range(12)) + [19, 20], TWINS, SAT + [1], [12, 13, 14, 15, 4, 24]]
# the second call on the same contexts: other lists, another number of them
LISTS_B = [[18, 16], [5, 6, 7, 8, 9, 10, 11, 24], [], [22, 12, 14]]


def _owners(n_points, world):
    """uneven shards: with 3 ranks the last holds four points, with 4 ranks the last holds none; the twins are split over ranks, two on one"""
    p = np.arange(n_points)
    if world == 1:
        return np.zeros(n_points, dtype=int)
    if world == 2:
        return np.where(p % 3 == 0, 0, 1)
    if world == 3:
        return np.where(np.isin(p, (16, 18, 13, n_points - 1)), 2, p % 2)
    return p % 3


def _set(ctx, k, dt, sparse, seqs, extra=0):
    cap = max(len(seqs) + extra, 1)
    hs = api.HistogramSet(ctx, k, dt, cap, sparse_entries=(2 * sum(len(s) for s in seqs) + 65536) if sparse else 0)
    if seqs:
        hs.build(seqs)
    return hs


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_round(ctxs, sets, lists, sparse):
    """one update round's column sums over len(sets) ranks: partial payloads, the host-side collective, nearest on every rank
    -> [(pos, dist, m_total)] per rank"""
    world, n = len(sets), len(lists[0])
    payloads = [api.colsum_partial(c, s, l) for c, s, l in zip(ctxs, sets, lists)]
    for r, p in enumerate(payloads):
        counts = [len(x) for x in lists[r]]
        if sparse:          # {n, bytes, (members, offset) x n}
            t = p[:16 + 16 * n].view(np.uint64)
            assert (int(t[0]), int(t[1])) == (n, p.size) and t[2::2].tolist() == counts, r
        else:               # ... then the member counts, the payload's last n words
            assert p.view(np.uint64)[-n:].tolist() == counts, r
    if sparse:
        each = up16(max(p.size for p in payloads))
        blob = np.zeros(world * each, dtype=np.uint8)
        for w, p in enumerate(payloads):
            blob[w * each: w * each + p.size] = p
    else:
        assert len({p.size for p in payloads}) == 1
        each = payloads[0].size
        total = np.zeros(each // 8, dtype=np.uint64)
        for p in payloads:
            total += p.view(np.uint64)
        blob = total.view(np.uint8)
    out = []
    for c, s, l in zip(ctxs, sets, lists):
        d = c.device_malloc(blob.size)          # world x bytes_per_rank (dense: the one reduced array)
        try:
            c.memcpy_to_device(d, blob)
            out.append(api.colsum_nearest(c, s, l, d, each, world))
        finally:
            c.device_free(d)
    return out


def _check_colsums(ctxs, seqs, k, dt, sparse, world, rounds, expect, seen):
    """rounds: global lists per call; expect[(call, list)] = (single-GPU distances, oracle distances); seen[(call, list, member)] = the
    distance any earlier world gave that member"""
    owner = _owners(len(seqs), world)
    local = [np.flatnonzero(owner == r) for r in range(world)]
    slot_of = {int(p): i for r in range(world) for i, p in enumerate(local[r][::-1] if r % 2 else local[r])}          # odd ranks: reversed
    sets = [_set(ctxs[r], k, dt, sparse, [seqs[p] for p in (local[r][::-1] if r % 2 else local[r])]) for r in range(world)]
    for call, glists in enumerate(rounds):
        mine = [[[j for j, p in enumerate(L) if owner[p] == r] for L in glists] for r in range(world)]
        lists = [[np.array([slot_of[glists[c][j]] for j in mine[r][c]], dtype=np.uint32) for c in range(len(glists))] for r in range(world)]
        got = _colsum_round(ctxs[:world], sets, lists, sparse)
        for c, L in enumerate(glists):
            recs = []
            for r in range(world):
                pos, dist, m_total = got[r][0][c], got[r][1][c], got[r][2][c]
                assert m_total == len(L), (world, call, c, r)
                js = mine[r][c]
                if not js:
                    assert pos == -1, (world, call, c, r)
                    continue
                gd, od = expect[(call, c)]
                want = int(np.argmin(gd[js]))          # first minimum among this rank's members, in their order
                assert pos == want and int(np.argmin(od[js])) == want, (world, call, c, r, pos, want)
                j = js[pos]
                assert dist == gd[j], (world, call, c, r, dist, gd[j])          # the single-GPU distance, bit for bit
                assert dist == pytest.approx(od[j], rel=1e-12, abs=0), (world, call, c, r)
                assert seen.setdefault((call, c, L[j]), dist) == dist, (world, call, c, r)
                recs.append((dist, j))
            if L:          # the driver's fold: smallest distance, then the earlier list position -- the single-GPU nearest member
                assert min(recs)[1] == int(np.argmin(expect[(call, c)][0])), (world, call, c)
    for s in sets:
        s.close()


def _expectations(ctx, oracle, seqs, k, dt, sparse, rounds):
    whole = _set(ctx, k, dt, sparse, seqs)
    oh = {}
    expect = {}
    for call, glists in enumerate(rounds):
        for c, L in enumerate(glists):
            if not L:
                continue
            pos, gd, _ = api.mean_nearest(ctx, whole, np.array(L, dtype=np.uint32))
            for p in L:
                if p not in oh:
                    oh[p] = oracle.hist(seqs[p], k, dt)
            _, od, opos = oracle.mean_nearest([oh[p] for p in L])
            assert pos == opos and np.allclose(gd, od, rtol=1e-12, atol=0), (call, c)
            expect[(call, c)] = (gd.copy(), od.copy())
    whole.close()
    for h in oh.values():
        oracle.lib().orc_hist_free(h)
    return expect


@pytest.mark.parametrize("k,dt,sparse", [(5, 16, False), (9, 8, False), (9, 8, True), (9, 32, False), (9, 32, True), (6, 64, False)])
def test_colsum_nearest_over_ranks(ranks, oracle, k, dt, sparse):
    """For N = 1..4 ranks and two calls in a row (other lists: the sparse accumulators must be zero again, on a rank without members
    too): every rank's nearest member is the first minimum of the oracle's distances among its own members, at the single-GPU distance
    bit for bit; the same member gets the same distance whatever N and whichever rank holds it; m_total is the list's size."""
    if dt == 8:
        assert max(oracle.hist(POOL[i], k, dt).array().max() for i in SAT) == 255          # the saturated bins are there
    rounds = [LISTS_A, LISTS_B]
    expect = _expectations(ranks[0], oracle, POOL, k, dt, sparse, rounds)
    seen = {}
    for world in (1, 2, 3, 4):
        _check_colsums(ranks, POOL, k, dt, sparse, world, rounds, expect, seen)


def test_colsum_nearest_k13_u64_sparse(ranks, oracle):
    """cfg4's shape (k = 13, uint64_t, 20 kb, sparse) with few members: a list of four split over up to four ranks, one member, empty"""
    seqs, _ = cfg4_sequences()
    rounds = [[[0, 1, 2, 4], [3], []], [[4, 2], [0, 3, 1]]]
    expect = _expectations(ranks[0], oracle, seqs, 13, 64, True, rounds)
    seen = {}
    for world in (1, 2, 3, 4):
        _check_colsums(ranks, seqs, 13, 64, True, world, rounds, expect, seen)


def test_colsum_errors(ranks):
    """a gathered table for another number of lists, decreasing offsets: MSC_ERR_INVALID_ARG, not a fault"""
    ctx = ranks[0]
    sp = _set(ctx, 9, 8, True, POOL[:6])
    blob = api.colsum_partial(ctx, sp, [[0, 1], [2]])
    d = ctx.device_malloc(up16(blob.size))
    try:
        ctx.memcpy_to_device(d, blob)
        with pytest.raises(MscError) as e:
            api.colsum_nearest(ctx, sp, [[0, 1], [2], [3]], d, up16(blob.size), 1)
        assert e.value.code == ERR_INVALID_ARG
        pos, _, m_total = api.colsum_nearest(ctx, sp, [[0, 1], [2]], d, up16(blob.size), 1)          # still usable
        assert m_total.tolist() == [2, 1] and pos[1] == 0
    finally:
        ctx.device_free(d)
    lib = ctx.lib
    slots = np.array([0, 1, 2], dtype=np.uint32)
    offs = np.array([0, 2, 1, 3], dtype=np.uint64)
    p, nb = C.c_void_p(), C.c_uint64()
    for s in (sp, _set(ctx, 5, 16, False, POOL[:6])):
        assert lib.msc_colsum_partial(ctx.h, s.h, api._ptr(slots), api._ptr(offs), 3, C.byref(p), C.byref(nb)) == ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ pack / unpack / reset
def _pack_image(ctx, hs, slots, one=False):
    """pack slots of hs at gapped offsets (multiples of 16) -> (host image, offsets); one=True: one msc_hist_pack call per slot"""
    offs, at = [], 32
    for i, s in enumerate(slots):
        offs.append(at)
        at += hs.packed_bytes(s) + 16 * (i % 3 + 1)
    d = ctx.device_malloc(at)
    try:
        ctx.memcpy_to_device(d, np.zeros(at, dtype=np.uint8))          # (pack leaves the 16-byte alignment padding of a range unwritten)
        if one:
            for s, o in zip(slots, offs):
                hs.pack([s], d, [o])
        else:
            hs.pack(slots, d, offs)
        img = ctx.memcpy_to_host(d, at)
    finally:
        ctx.device_free(d)
    return img, offs


def _on_device(ctx, img):
    d = ctx.device_malloc(img.size)
    ctx.memcpy_to_device(d, img)
    return d


def _same_slot(a, sa, b, sb):
    assert np.array_equal(a.download(sa), b.download(sb)), (sa, sb)
    assert a.info(sa) == b.info(sb), (sa, sb)


def _scores_alike(ctx, trn, feat, hs, s, d, n):
    """slot d scores bit for bit as slot s of the same set: as query and candidate of score_multi, get_close, filter and closest"""
    base = [i for i in range(n) if i != s]
    cands = np.array(base[:5] + [s] + base[5:] + [d], dtype=np.uint32)
    r = api.score_multi(ctx, feat, hs, cands, hs, [s, d, 2], feat_mask=ALL_MASK)
    for key in ("sum", "csum", "close", "raw"):
        assert np.array_equal(r[key][0], r[key][1]), key
        assert np.array_equal(r[key][:, 5], r[key][:, -1]), key
    others = np.array(base, dtype=np.uint32)
    g_s, g_d = trn.get_close(hs, others, hs, s), trn.get_close(hs, others, hs, d)
    assert np.array_equal(g_s[0], g_d[0]) and g_s[1:] == g_d[1:]
    with_s, with_d = np.array(base[:4] + [s] + base[4:], dtype=np.uint32), np.array(base[:4] + [d] + base[4:], dtype=np.uint32)
    g_s, g_d = trn.get_close(hs, with_s, hs, 1), trn.get_close(hs, with_d, hs, 1)
    assert np.array_equal(g_s[0], g_d[0]) and g_s[1:] == g_d[1:]
    assert np.array_equal(trn.filter(hs, s, hs, others), trn.filter(hs, d, hs, others))
    assert np.array_equal(trn.filter(hs, 1, hs, with_s), trn.filter(hs, 1, hs, with_d))
    p_s, d_s, _ = trn.closest(hs, with_s[:8])
    p_d, d_d, _ = trn.closest(hs, with_d[:8])
    assert p_s == p_d and np.array_equal(d_s, d_d)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_pack_unpack_exact_copies(ranks, sparse):
    """pack on one rank (both paths), unpack on another at other slots (one-slot path, batched path with consecutive and scattered
    slots) over slots the destination's mirrors / rank-list cache already cover: exact copies (stale magnitude included) that score as
    their source"""
    k, dt = 9, 8
    A_ctx, B_ctx = ranks[0], ranks[1]
    n = len(POOL)
    st = n - 1          # slot 24 (the short sequence) becomes a slot with a stale magnitude
    A = _set(A_ctx, k, dt, sparse, POOL)
    A.assign_from(st, A, 2)
    assert A.info(st)["mag"] != A.info(2)["mag"]
    for s in range(n):
        assert A.packed_bytes(s) % 16 == 0 and A.packed_bytes(s) > 0
    src = [st, 3, 0, 19, 12, 5, 21]
    img, offs = _pack_image(A_ctx, A, src)
    img1, offs1 = _pack_image(A_ctx, A, src, one=True)
    assert offs == offs1
    for s, o in zip(src, offs):          # the one-slot and the batched pack write the same bytes
        assert np.array_equal(img[o:o + A.packed_bytes(s)], img1[o:o + A.packed_bytes(s)]), s
    # the destination: the same points, plus 8 extra slots already holding other histograms
    extra = 8
    B = _set(B_ctx, k, dt, sparse, POOL, extra)
    B.assign_from(st, B, 2)
    B.build(POOL[6:6 + extra], first_slot=n)
    feat = api.Feature.from_text(B_ctx, weights_text("weights_cfg5_k9.txt"), 0)          # `--feat slow`: the divergence mirrors
    trn = api.Trainer(B_ctx, feat, 0.6)
    everyone = np.arange(n + extra, dtype=np.uint32)
    api.score_multi(B_ctx, feat, B, everyone, B, everyone, feat_mask=ALL_MASK)          # Q x M: presence-bit / ranks / sparse mirrors
    for _ in range(3):          # a sparse set's rank-list cache is built on the third request
        trn.get_close(B, everyone[1:], B, 0)
    dev = _on_device(B_ctx, img)
    try:
        dst = {st: n + 5, 3: n, 0: n + 1, 19: n + 2, 12: n + 7, 5: n + 3, 21: n + 4}
        B.unpack([dst[s] for s in src[1:4]], dev, offs[1:4])          # batched, consecutive slots
        B.unpack([dst[12], dst[21]], dev, [offs[4], offs[6]])          # batched, scattered slots in descending order
        B.unpack([dst[5]], dev, [offs[5]])          # one slot
        B.unpack([dst[st]], dev, [offs[0]])          # one slot, stale magnitude
    finally:
        B_ctx.device_free(dev)
    for s in src:
        _same_slot(A, s, B, dst[s])
        _same_slot(B, s, B, dst[s])
    for s in src:
        _scores_alike(B_ctx, trn, feat, B, s, dst[s], n)


def test_pack_unpack_over_a_built_rank_list_cache_without_reset(ranks):
    """sparse: unpack (no reset) over a slot of a set whose rank-list cache is built; the next get_close sees the new slot"""
    ctx = ranks[2]
    n = len(POOL)
    B = _set(ctx, 9, 8, True, POOL)
    feat = api.Feature.from_text(ctx, weights_text("weights_k9_u32.txt"), 0)
    trn = api.Trainer(ctx, feat, 0.9)
    cands = np.array([i for i in range(n) if i not in (7, 20)], dtype=np.uint32)
    for _ in range(3):
        trn.get_close(B, cands, B, 7)
    img, offs = _pack_image(ctx, B, [20])
    dev = _on_device(ctx, img)
    try:
        B.unpack([9], dev, offs)          # slot 9 (a relative of the query) now holds sequence 20
    finally:
        ctx.device_free(dev)
    B2 = _set(ctx, 9, 8, True, POOL[:9] + [POOL[20]] + POOL[10:])
    exp = trn.get_close(B2, cands, B2, 7), api.score_multi(ctx, feat, B2, cands, B2, [7], feat_mask=api.FEAT_FAST)
    got = trn.get_close(B, cands, B, 7), api.score_multi(ctx, feat, B, cands, B, [7], feat_mask=api.FEAT_FAST)
    assert np.array_equal(got[0][0], exp[0][0]) and got[0][1:] == exp[0][1:]
    for key in ("sum", "close", "raw"):          # (the candidate shorter than k has NaN statistics)
        assert np.array_equal(got[1][key], exp[1][key], equal_nan=True), key


@pytest.mark.parametrize("after", [None, "1"], ids=["cache_at_third", "cache_at_first"])
def test_install_query_loop(ranks, monkeypatch, after):
    """the driver's install_query: reset a one-slot sparse staging set, unpack the broadcast query into slot 0, get_close against the
    points -- three times per query, so that the rank-list cache exists when the next reset / unpack must make it stale"""
    if after:
        monkeypatch.setenv("MSC_RANKS_1XM_AFTER", after)
    A_ctx, B_ctx = ranks[0], ranks[3]
    n = len(POOL)
    A = _set(A_ctx, 9, 8, True, POOL)
    B = _set(B_ctx, 9, 8, True, POOL)
    stage = api.HistogramSet(B_ctx, 9, 8, 1, sparse_entries=max(A.entries(s) for s in range(n)) + 16)
    feat = api.Feature.from_text(B_ctx, weights_text("weights_k9_u32.txt"), 0)
    trn = api.Trainer(B_ctx, feat, 0.9)
    cands = np.arange(n, dtype=np.uint32)
    for q in (0, 7, 19, 12, 3, 15):
        img, offs = _pack_image(A_ctx, A, [q])
        dev = _on_device(B_ctx, img)
        try:
            stage.reset()
            stage.unpack([0], dev, offs)
        finally:
            B_ctx.device_free(dev)
        _same_slot(stage, 0, A, q)
        exp = trn.get_close(B, cands, B, q)
        for _ in range(3):
            got = trn.get_close(B, cands, stage, 0)
            assert np.array_equal(got[0], exp[0]) and got[1:] == exp[1:], q
            rev = trn.get_close(stage, [0], B, q)          # the staged slot as the candidate
            own = trn.get_close(B, [q], B, q)
            assert np.array_equal(rev[0], own[0]) and rev[1:] == own[1:], q


def test_unpack_errors(ranks):
    """wrong layout, a dense or sparse slot of another k or bin type: MSC_ERR_INVALID_ARG; a full arena: MSC_ERR_OOM, the set still
    usable; decreasing offsets are refused -- all caught on the host"""
    ctx = ranks[0]
    dense = _set(ctx, 9, 8, False, POOL[:4])
    sparse = _set(ctx, 9, 8, True, POOL[:4])

    def image(hs, slots):
        img, offs = _pack_image(ctx, hs, slots)
        return _on_device(ctx, img), offs

    def refused(hs, slots, dev, offs, code):
        with pytest.raises(MscError) as e:
            hs.unpack(slots, dev, offs)
        assert e.value.code == code, (slots, e.value)

    bufs = []
    try:
        d_dense, o_dense = image(dense, [0, 1])
        d_sparse, o_sparse = image(sparse, [0, 1])
        bufs += [d_dense, d_sparse]
        for one in (True, False):          # the one-slot and the batched path
            sl = slice(0, 1) if one else slice(0, 2)
            refused(sparse, [2, 3][sl], d_dense, o_dense[sl], ERR_INVALID_ARG)
            refused(dense, [2, 3][sl], d_sparse, o_sparse[sl], ERR_INVALID_ARG)
            for k, dt in ((9, 32), (8, 8), (10, 8)):          # another bin type, another k
                other_d = _set(ctx, k, dt, False, [], extra=2)
                refused(other_d, [0, 1][sl], d_dense, o_dense[sl], ERR_INVALID_ARG)
                other_s = _set(ctx, k, dt, True, [], extra=2)
                refused(other_s, [0, 1][sl], d_sparse, o_sparse[sl], ERR_INVALID_ARG)
                other_d.close()
                other_s.close()
        # a full arena
        small = api.HistogramSet(ctx, 9, 8, 4, sparse_entries=sparse.entries(0) + sparse.entries(1) // 2)
        small.unpack([0], d_sparse, o_sparse[:1])
        refused(small, [1], d_sparse, o_sparse[1:2], ERR_OOM)
        refused(small, [1, 2], d_sparse, o_sparse, ERR_OOM)
        small.reset()
        small.unpack([3], d_sparse, o_sparse[1:2])          # usable again
        _same_slot(small, 3, sparse, 1)
        # decreasing offsets in msc_filter_batch's lists (msc_colsum_partial's: test_colsum_errors)
        feat = api.Feature.from_text(ctx, weights_text("weights_k9_u32.txt"), 0)
        slots = np.array([0, 1, 2], dtype=np.uint32)
        offs = np.array([0, 2, 1, 3], dtype=np.uint64)
        keep = np.zeros(3, dtype=np.uint8)
        cs = np.array([0, 1, 2], dtype=np.uint32)
        assert ctx.lib.msc_filter_batch(ctx.h, feat.h, 0.9, dense.h, api._ptr(cs), 3, dense.h, api._ptr(slots), api._ptr(offs), api._ptr(keep)) == ERR_INVALID_ARG
    finally:
        for b in bufs:
            ctx.device_free(b)


# ------------------------------------------------------------------------------------------------ msc_filter_batch
FILTER_CASES = [(1, "weights_k9_u32.txt", 32, 0.9), (37, "weights_k9_u32.txt", 32, 0.9), (300, "weights_k9_u32.txt", 32, 0.9),
                (1, "weights_cfg5_k9.txt", 8, 0.6), (37, "weights_cfg5_k9.txt", 8, 0.6), (300, "weights_cfg5_k9.txt", 8, 0.6)]


@pytest.fixture(scope="module")
def filter_oracle(oracle):
    """oracle.filter_ of every (centre point, point) pair of the pool, per model"""
    out = {}
    for wts, dt, cutoff in {(w, d, c) for _, w, d, c in FILTER_CASES}:
        pred = oracle.predictor(weights_text(wts))
        oh = [oracle.hist(s, 9, dt) for s in POOL]
        out[wts] = np.array([oracle.filter_(pred, cutoff, oh[c], oh) for c in range(len(POOL))])
        for h in oh:
            oracle.lib().orc_hist_free(h)
    return out


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("nc,wts,dt,cutoff", FILTER_CASES)
def test_filter_batch(ranks, filter_oracle, sparse, nc, wts, dt, cutoff):
    """msc_filter_batch == one Trainer::filter per centre == oracle.filter_: centres from a separate set, empty lists, lists holding the
    centre's own point, slots repeated across lists"""
    ctx = ranks[1]
    n = len(POOL)
    rng = np.random.default_rng(nc * 7 + dt)
    pts = _set(ctx, 9, dt, sparse, POOL)
    owner = rng.integers(0, n - 1, nc)          # centre c is a copy of point owner[c] (not of the one shorter than k)
    cen = api.HistogramSet(ctx, 9, dt, nc + 3, sparse_entries=(sum(len(POOL[o]) for o in owner) + 65536) if sparse else 0)
    cslots = rng.permutation(nc + 3)[:nc].astype(np.uint32)
    cen.clone_batch(cslots, pts, owner.astype(np.uint32))
    lists = []
    for c in range(nc):
        m = int(rng.integers(0, 9))
        lst = list(rng.integers(0, n, m))
        if c % 4 == 1:
            lst.insert(int(rng.integers(0, m + 1)), int(owner[c]))          # the centre's own point
        if c % 5 == 2:
            lst = []
        lists.append(np.array(lst, dtype=np.uint32))
    if nc > 1:
        lists[-1] = lists[0].copy()          # the same slots in two lists
    feat = api.Feature.from_text(ctx, weights_text(wts), 0)
    trn = api.Trainer(ctx, feat, cutoff)
    keep = trn.filter_batch(cen, cslots, pts, lists)
    kept = 0
    for c in range(nc):
        one = trn.filter(cen, int(cslots[c]), pts, lists[c]) if lists[c].size else np.zeros(0, dtype=np.uint8)
        assert np.array_equal(keep[c], one), c
        assert np.array_equal(keep[c], filter_oracle[wts][owner[c]][lists[c]]), c
        kept += int(keep[c].sum())
    if nc >= 37:
        total = sum(x.size for x in lists)
        assert 0 < kept < total          # both decisions occur
