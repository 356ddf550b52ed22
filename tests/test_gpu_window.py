"""msc_get_close_window (csrc/msc_window.hip) against a CPU model of the window (tests/window_model.py) that stands on the oracle's verdicts.

msc_window_create takes an order that names a slot more than once, so a window of a million positions over four dozen small histograms costs
milliseconds, holds exact ties by construction, and needs ONE oracle verdict per distinct histogram and query. Every step here asserts, exactly:
the alive count, the close positions, the best position and is_min; the best similarity at rel = 1e-8 to the oracle's; and, where the range
holds at most 20 000 alive positions, the same against Trainer.get_close over order[pos], bit for bit. What the steps aim at:

  - the three compaction forms at the edges of their ranges (Window.last_compaction says which one ran), the fused reduce through more than
    four sweeps of its 1 024 parts and the unfused one at its cap of 256 parts;
  - the tie rule (equal similarities: the lowest window position), which is what makes the claim order of the multi-block list harmless;
  - tiles without an alive position, kills in the kernel's arguments and in the page-locked list, kills outside the range, kills left pending by
    a call that returned early, and the three refusals of msc_window_kill;
  - both reduce routes: MSC_NO_FUSED_REDUCE, read on every call, sends a window pass through k_pair_epilogue, the keyed k_pair_reduce* and
    k_window_close (Window.last_close_blocks counts the workgroups of that last one; 0 on the fused route).

The tie tests fail where the tie rule breaks: every one runs at first = 2 047 with a dead position in front of the winner, so a best "position"
that is an index into the compacted list (`c` for `cl.pos[c]` in k_pair_epilogue_reduce_part, or no `key` in msc_launch_reduce) is another
number than the asserted one."""
import numpy as np
import pytest

from golden_util import weights_text
from meshclust2_amd import api, synth
from window_model import WindowModel, check_separation, oracle_verdict

pytestmark = pytest.mark.gpu

# msc_get_close_window's switches between its compaction forms (csrc/msc_window.hip: kWinBlock, kWinPer and the two tests of `range`)
ONE_BLOCK_MAX = 4096             # up to here k_window_compact_one, one workgroup of 1 024 threads
SMALL_TILE = 2048                # above: k_window_compact with 256 threads, 8 positions a thread ...
SMALL_TILE_MAX = 524288          # ... up to here (64 tiles of the large form)
LARGE_TILE = 8192                # above: 1 024 threads, 8 positions a thread
# the reduce (csrc/pair_features.hip): the fused form sweeps 1 024 parts of 256 candidates, msc_launch_reduce caps its parts at 256 of 4 096
FUSED_SWEEP = 1024 * 256
UNFUSED_CAP = 256 * 4096
COMPARE_MAX = 20000              # alive positions up to which a step is also held to Trainer.get_close, bit for bit
BIG = 1100000

K, DTYPE, CUTOFF, WEIGHTS = 5, 16, 0.9, "weights_k5_u16.txt"
N_SLOTS = 48                     # the slots an order draws from; the set holds query-only sequences behind them
RARE = 46                        # a sequence unrelated to the rest, drawn rarely: a query that is close to few positions
LONER = 48                       # query only: unrelated to every slot, so it scores its length window and is close to nothing


def sequences():
    """48 sequences of 300 .. 1 000 bases: five families of eight around 800 bases (slots 0 and 1 hold the SAME sequence), three cut short and
    two spliced long -- outside the length window [qlen * 0.9, qlen / 0.9] of the families' queries --, two unrelated ones; then the loner"""
    fam, _ = synth.families(7301, 40, 800, family=8, length_jitter=60)
    odd, _ = synth.families(7302, 3, 800, family=1, length_jitter=40)
    seqs = [fam[0], fam[0]] + fam[1:40]
    seqs += [fam[8][:300], fam[16][:380], fam[24][:450], (fam[9] + fam[17])[:1000], (fam[25] + fam[33])[:960]]
    seqs += odd[:2]
    assert len(seqs) == N_SLOTS and seqs[0] == seqs[1] and all(300 <= len(s) <= 1000 for s in seqs)
    return seqs + [odd[2]]


def draw_order(seed, n):
    """a seeded draw with replacement from the slots: slot 10 heavy (a tenth of the positions), RARE at 4 in 1 000, the rest alike"""
    w = np.ones(N_SLOTS)
    w[10] = 0.1 * (N_SLOTS - 2) / 0.896
    w[RARE] = 0.004 * (N_SLOTS - 2) / 0.896
    return np.random.default_rng(seed).choice(N_SLOTS, size=n, p=w / w.sum()).astype(np.uint32)


class World:
    """a context, a histogram set, a model on the device and in the oracle, and the oracle's verdict per query"""

    def __init__(self, oracle, seqs, k, dtype, weights, cutoff, n_slots, copies, sparse=False):
        self.oracle, self.n_slots, self.cutoff, self.copies = oracle, n_slots, cutoff, copies
        self.ctx = api.Context(0)
        self.hs = api.HistogramSet(self.ctx, k, dtype, len(seqs), sparse_entries=(sum(len(s) for s in seqs) + 4096) if sparse else 0)
        self.hs.build(seqs)
        self.feat = api.Feature.from_text(self.ctx, weights_text(weights), 0)
        self.trn = api.Trainer(self.ctx, self.feat, cutoff)
        self.pred = oracle.predictor(weights_text(weights))
        self.oh = [oracle.hist(s, k, dtype) for s in seqs]
        self._verdicts = {}

    def verdict(self, q):
        if q not in self._verdicts:
            v = oracle_verdict(self.oracle, self.pred, self.cutoff, self.oh[q], self.oh[:self.n_slots])
            check_separation(v, self.copies)
            self._verdicts[q] = v
        return self._verdicts[q]

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def world(oracle):
    w = World(oracle, sequences(), K, DTYPE, WEIGHTS, CUTOFF, N_SLOTS, copies=[(0, 1)])
    yield w
    w.close()


@pytest.fixture(params=["fused", "unfused"])
def route(request, monkeypatch):
    """the library reads the switch on every call"""
    monkeypatch.delenv("MSC_NO_FUSED_REDUCE", raising=False)
    if request.param == "unfused":
        monkeypatch.setenv("MSC_NO_FUSED_REDUCE", "1")
    return request.param


def expected_form(length, n_alive):
    if n_alive == 0:
        return (0, 0)
    if length <= ONE_BLOCK_MAX:
        return (1, 1024)
    if length <= SMALL_TILE_MAX:
        return (-(-length // SMALL_TILE), 256)
    return (-(-length // LARGE_TILE), 1024)


class Pair:
    """a device window and its model, stepped together"""

    def __init__(self, world, order):
        self.w, self.order = world, np.ascontiguousarray(order, dtype=np.uint32)
        self.win = api.Window(world.ctx, world.hs, self.order)
        self.mdl = WindowModel(self.order)
        self.n = self.order.size

    def counts(self, *ranges):
        for a, b in ((0, self.n),) + ranges:
            assert self.win.alive(a, b) == self.mdl.alive(a, b), (a, b)

    def kill(self, positions):
        self.mdl.kill(positions)
        self.win.kill(positions)

    def refused(self, positions):
        """a call msc_window_kill refuses as a whole: the model refuses it too, and the counts stay"""
        before = self.mdl.alive()
        with pytest.raises(ValueError):
            self.mdl.kill(positions)
        with pytest.raises(api.MscError):
            self.win.kill(positions)
        assert self.win.alive() == before == self.mdl.alive()

    def step(self, q, a, b, route=None, form=None):
        """one get_close over [a, b) on both; -> (close, best_pos, best_sim, is_min) of the device"""
        w, what = self.w, (q, a, b, route)
        v = w.verdict(q)
        pos = self.mdl.alive_positions(a, b)
        assert self.win.alive(a, b) == pos.size, what
        close, bp, bs, im = self.win.get_close(w.trn, a, b, w.hs, q)
        launched, launches, close_blocks = self.win.last_compaction(), w.ctx.last_kernel_launches(), self.win.last_close_blocks()
        mclose, mbp, mbs, mim, n_alive = self.mdl.get_close(v, a, b)
        assert n_alive == pos.size
        assert np.array_equal(close, mclose), (what, close[:8], mclose[:8], close.size, mclose.size)
        assert (bp, im) == (mbp, mim), what
        assert bs == (pytest.approx(mbs, rel=1e-8) if mbp >= 0 else -1.0), what
        assert launched == expected_form(min(b, self.n) - a if a < min(b, self.n) else 0, n_alive), what
        if form is not None:
            assert launched == form, what
        if n_alive and route is not None:
            # one pass kernel on either route; the close pass is a kernel of its own only behind the unfused reduce
            assert launches == 1 and close_blocks == (0 if route == "fused" else -(-n_alive // 256)), (what, launches, close_blocks)
        if 0 < n_alive <= COMPARE_MAX:
            flags, tbp, tbs, tim = w.trn.get_close(w.hs, self.order[pos], w.hs, q)
            assert np.array_equal(close, pos[np.flatnonzero(flags)]), what
            assert bp == (int(pos[tbp]) if tbp >= 0 else -1) and im == tim and (tbp < 0 or bs == tbs), what
        assert self.win.alive(a, b) == self.mdl.alive(a, b) and self.win.alive() == self.mdl.alive(), what
        return close, bp, bs, im

    def close(self):
        self.win.close()


def test_the_model_is_small_enough_for_the_fused_reduce(world, monkeypatch):
    """histograms of at most four tiles: the fused epilogue + reduce kernel is the default, MSC_NO_FUSED_REDUCE the way to the other route.
    Both run ONE pass kernel (last_kernel_launches counts those), so the routes are told apart by the close pass: inside the fused kernel, or
    k_window_close behind the keyed reduce."""
    monkeypatch.delenv("MSC_NO_FUSED_REDUCE", raising=False)
    p = Pair(world, draw_order(1, 9000))
    p.step(LONER, 0, 9000, route="fused")
    assert p.win.last_close_blocks() == 0
    monkeypatch.setenv("MSC_NO_FUSED_REDUCE", "1")
    p.step(LONER, 0, 9000, route="unfused")          # 9 000 candidates: past the 8 192 of the one-workgroup reduce as well
    p.step(3, 100, 8000, route="unfused")            # ... and under it
    v = world.verdict(LONER)
    assert v.scored.sum() > 20 and not v.close.any() and not v.scored.all()          # the loner scores a length window and kills nothing
    v = world.verdict(3)
    assert v.close.sum() >= 5 and (v.scored & ~v.close).sum() >= 5 and (~v.scored).sum() >= 5
    p.close()


QUERIES = [3, 12, 20, 28, 36, 0, 44, 41, RARE, 47, LONER]          # a member of each family, a copy, a long and a short one, the unrelated ones


@pytest.mark.parametrize("first", [0, 2047])
def test_range_edges(world, route, first):
    """every length at which the compaction changes its form or a tile fills up, at an aligned and an unaligned start"""
    p = Pair(world, draw_order(2, BIG))
    # the short ranges first, each at a start of its own: they take little from the window, and the long ones do not empty them
    for i, (length, form) in enumerate(((6145, (4, 256)), (6144, (3, 256)), (4097, (3, 256)), (4096, (1, 1024)), (4095, (1, 1024)), (1025, (1, 1024)),
                                        (1024, (1, 1024)), (1023, (1, 1024)), (65, (1, 1024)), (64, (1, 1024)), (63, (1, 1024)), (1, (1, 1024)))):
        a = first + 8192 * (1 + i)
        q = int(p.order[a]) if length < 64 else QUERIES[i % len(QUERIES)]          # (a query the shortest ranges hold a copy of)
        p.step(q, a, a + length, route, form=form)
        p.step(LONER, a, a + length, route, form=form if p.mdl.alive(a, a + length) else (0, 0))          # the same range again, its close ones dead
    if first == 0:
        # the whole window, nearly all of it alive: RARE's few positions are the close ones of the first pass, and the second still holds
        # more than four sweeps of the fused reduce's parts and more than the unfused one's 256 parts take at 4 096 each
        for q, length, blocks in ((RARE, BIG, 135), (LONER, BIG, 135), (3, 540000, 66), (12, 532480, 65), (20, 524289, 65)):
            if length == BIG:
                assert p.mdl.alive(0, length) > max(4 * FUSED_SWEEP, UNFUSED_CAP)
            close, _, _, _ = p.step(q, 0, length, route, form=(blocks, 1024))
            assert close.size > 1000 or q == LONER
    close, _, _, _ = p.step(28, first, first + 524288, route, form=(256, 256))
    assert close.size > 1000
    p.counts((first, first + 4096), (first + 1, BIG - 1))
    p.close()


def _first_of(order, live, slots, a, b):
    at = a + np.flatnonzero(live[a:b] & np.isin(order[a:b], slots))
    return int(at[0]) if at.size else -1


FORMS = {"one": (20000, 4000, (1, 1024)), "256": (40000, 3 * SMALL_TILE + 77, (4, 256)), "1024": (BIG, SMALL_TILE_MAX + 1, (65, 1024))}


def _tie_scenario(world, form, route):
    """-> everything the device returned, step by step"""
    n, length, grid = FORMS[form]
    p = Pair(world, draw_order(3, n))
    order, a, out = p.order, 2047, []
    b = a + length
    v = world.verdict(LONER)
    top = int(np.argmax(np.where(v.scored, v.sim, -np.inf)))          # the loner's best slot: scored, not close, thousands of copies
    assert not v.close[top] and np.count_nonzero(order[a:b] == top) >= 3
    assert np.count_nonzero(v.scored & (v.sim == v.sim[top])) == 1
    # a dead position in front of the range's first copy and one at the range's start: an index into the list is not a position
    p1 = _first_of(order, p.mdl.live, [top], a, b)
    p.kill([a, p1 - 1] if p1 - 1 > a else [a])
    for _ in range(3):          # the lowest alive copy wins; it is killed; the next one wins
        pw = _first_of(order, p.mdl.live, [top], a, b)
        got = p.step(LONER, a, b, route, form=grid)
        assert got[1] == pw and order[pw] == top and got[0].size == 0
        out.append(got)
        p.kill([pw])
    # the two copies of one sequence, slots 0 and 1, tie across slots: in a range that starts at a copy in slot 1 that position wins, in one
    # that starts at a copy in slot 0 that one (the query is the sequence itself; its copies are close, so they die with the call)
    v0 = world.verdict(0)
    best = np.where(v0.scored, v0.sim, -np.inf)
    assert sorted(np.flatnonzero(best == best.max()).tolist()) == [0, 1] and v0.close[0] and v0.close[1]
    s1 = _first_of(order, p.mdl.live, [1], 0 if form == "1024" else b, n)          # (two ranges of 524 289 positions in 1 100 000: from the front)
    s0 = _first_of(order, p.mdl.live, [0], s1 + length, n)
    assert 0 <= s1 < s0 and s0 + length <= n
    for slot, s in ((1, s1), (0, s0)):
        got = p.step(0, s, s + length, route, form=grid)
        assert got[1] == s and order[s] == slot and got[0].size >= 2 and got[0][0] == s
        assert {0, 1} <= set(order[got[0]].tolist())          # copies in both slots were in the range
        out.append(got)
    assert len(out) == 5
    p.counts((a, b))
    p.close()
    return out


@pytest.mark.parametrize("form", ["one", "256", "1024"])
def test_ties_go_to_the_lowest_alive_position(world, route, form):
    one = _tie_scenario(world, form, route)
    two = _tie_scenario(world, form, route)          # a fresh window, the same steps: the same returns whatever order the tiles' claims landed in
    for x, y in zip(one, two):
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:]


@pytest.mark.parametrize("form", ["256", "1024"])
def test_dead_tiles(world, route, form):
    n, _, _ = FORMS[form]
    tile = SMALL_TILE if form == "256" else LARGE_TILE
    tiles = 5 if form == "256" else 65
    a = 2047
    b = a + tiles * tile - 100          # the last tile is not full
    grid = (tiles, 256 if form == "256" else 1024)
    p = Pair(world, draw_order(4, n))
    mid = tiles // 2
    p.kill(np.arange(a + mid * tile, a + (mid + 1) * tile))          # one whole tile
    p.step(3, a, b, route, form=grid)
    p.kill(p.mdl.alive_positions(a, a + tile))                       # the first tile, what is left of it
    p.step(12, a, b, route, form=grid)
    p.kill(p.mdl.alive_positions(a + (tiles - 1) * tile, b))         # the last tile
    p.step(20, a, b, route, form=grid)
    assert p.mdl.alive(a, a + tile) == p.mdl.alive(a + mid * tile, a + (mid + 1) * tile) == p.mdl.alive(a + (tiles - 1) * tile, b) == 0
    p.step(28, a, b - 3 * tile, route)                                # a range that starts with a dead tile
    # a second range of the same shape, untouched so far: everything dies but its last position
    a = 20000 if form == "256" else 540000
    b = a + tiles * tile - 100
    assert b <= n and p.mdl.alive(a, b) == b - a
    last = b - 1
    q_last = int(p.order[last])
    p.kill(p.mdl.alive_positions(a, last))
    assert p.mdl.alive(a, b) == 1
    close, bp, _, _ = p.step(LONER, a, b, route, form=grid)
    assert close.size == 0 and bp == (last if world.verdict(LONER).scored[q_last] else -1)
    close, bp, _, im = p.step(q_last, a, b, route, form=grid)       # its own sequence: close, and it dies
    assert close.tolist() == [last] and bp == last and not im
    # nothing alive: the call returns empty before it launches anything
    close, bp, bs, im = p.step(3, a, b, route, form=(0, 0))
    assert close.size == 0 and (bp, bs, im) == (-1, -1.0, True) and p.win.last_compaction() == (0, 0) and p.win.last_close_blocks() == 0
    p.step(3, 0, n if form == "256" else a + tile, route)             # the positions around the range are as they were
    p.close()


@pytest.mark.parametrize("form", ["one", "256"])
def test_kills(world, route, form):
    n = 60000
    length = 4000 if form == "one" else 3 * SMALL_TILE + 5
    grid = (1, 1024) if form == "one" else (4, 256)
    tile = SMALL_TILE
    p = Pair(world, draw_order(5, n))
    rng = np.random.default_rng(55)
    a = 2047
    b = a + length

    def some(count, lo, hi):
        return rng.choice(p.mdl.alive_positions(lo, hi), size=count, replace=False)

    # four kills travel in the kernel's arguments, five in the page-locked list
    p.kill(some(4, a, b))
    p.step(3, a, b, route, form=grid)
    p.kill(some(5, a, b))
    p.step(12, a, b, route, form=grid)
    # the first and the last position of a tile, of the range, and the positions either side of the range
    edge = [x for x in (a, a + tile - 1, a + tile, a + 2 * tile - 1, a + 2 * tile, b - 1, a - 1, b) if p.mdl.live[x]]
    assert len(edge) >= 5
    p.kill(edge)
    p.step(20, a, b, route, form=grid)
    assert all(p.win.alive(x, x + 1) == 0 for x in edge)
    # kills outside the next range only (in front of it and behind it): 3, then 7; a later range holds them, dead
    for count in (3, 7):
        out = np.concatenate([some(count - count // 2, 0, a - 1), some(count // 2, b + 1, b + 3000)])
        p.kill(out)
        p.step(28, a, b, route, form=grid)
        close, _, _, _ = p.step(36, 0, b + 3000, route)
        assert not np.isin(out, close).any() and all(p.win.alive(int(x), int(x) + 1) == 0 for x in out)
    # more kills in one call than the list's first buffer of 4 096 entries holds, then more than its second
    a2 = 20000
    b2 = a2 + length
    p.kill(np.concatenate([some(2500, a2 + length, n), some(1500, a2, b2), some(1000, 0, a2)]))
    p.step(3, a2, b2, route, form=grid)
    p.kill(np.concatenate([some(9000, b2, n), some(1000, a2, b2), some(2000, 0, a2)]))
    p.step(12, a2, b2, route, form=grid)
    p.step(20, 0, n, route)
    p.counts((a2, b2), (0, a2), (b2, n))
    # kills, then a call over a range with nothing alive in it (it returns early, the kills stay on file), then a range that holds them
    a3 = 40000
    b3 = a3 + length
    p.kill(p.mdl.alive_positions(a3 + 10, a3 + 200))
    pend = some(6, a3 + 200, b3)
    p.kill(pend)
    close, bp, _, im = p.step(3, a3 + 10, a3 + 200, route, form=(0, 0))
    assert close.size == 0 and bp == -1 and im
    close, _, _, _ = p.step(0, a3, b3, route, form=grid)
    assert not np.isin(pend, close).any() and p.win.alive(a3 + 10, a3 + 200) == 0
    p.step(LONER, a3, b3, route, form=grid)
    # the three refusals; each leaves the counts as they were (a good position is listed first every time) and the next pass correct
    good = int(p.mdl.alive_positions(a3, b3)[0])
    dead_by_kill, dead_by_close = int(pend[0]), int(close[0])
    for bad in ([good, n], [good, 0xfffffff0], [good, good], [good, dead_by_kill], [good, dead_by_close], [dead_by_close]):
        p.refused(np.array(bad, dtype=np.uint32))
        assert p.win.alive(good, good + 1) == 1
        p.step(QUERIES[len(bad) + bad[-1] % 5], a3, b3, route, form=grid)
    p.kill([good])
    p.refused([good])
    p.step(3, 0, n, route)
    p.close()


def test_small_api_edges(world, route):
    # a window of no positions
    e = Pair(world, np.zeros(0, dtype=np.uint32))
    assert e.win.alive() == 0 and e.win.alive(0, 5) == 0
    for a, b in ((0, 0), (0, 5), (3, 2)):
        close, bp, bs, im = e.step(3, a, b, route, form=(0, 0))
        assert close.size == 0 and (bp, bs, im) == (-1, -1.0, True)
    e.win.kill(np.zeros(0, dtype=np.uint32))
    e.refused([0])
    e.close()
    n = 30000
    p, r = Pair(world, draw_order(6, n)), Pair(world, draw_order(7, 5000))
    # first >= end, and an end past the window's
    for a, b in ((7, 7), (9, 3), (n, n + 5), (n + 1, n)):
        close, bp, bs, im = p.step(3, a, b, route, form=(0, 0))
        assert close.size == 0 and (bp, bs, im) == (-1, -1.0, True)
    assert p.win.alive(n - 10, n + 10) == 10 and p.win.alive(5, 5) == 0 and p.win.alive(9, 3) == 0
    p.step(3, n - 100, n + 100, route, form=(1, 1024))
    p.step(12, n - 5000, 2 * n, route, form=(3, 256))
    # two windows on one context, in turn: each keeps its own flags, counters and lists
    for i, q in enumerate(QUERIES):
        a = 400 * i
        p.step(q, a, a + 4500, route, form=(3, 256))
        r.kill(r.mdl.alive_positions(a, a + 3))
        r.step(q, a // 2, a // 2 + 900, route, form=(1, 1024))
    p.counts()
    r.counts()
    p.close()
    r.close()
    # a close list longer than the page-locked buffer the call before left: 4 096 entries after a short range, then a tenth of 60 000 positions
    g = Pair(world, draw_order(8, 60000))
    g.step(3, 10, 30, route, form=(1, 1024))
    close, bp, _, _ = g.step(10, 0, 60000, route, form=(30, 256))
    assert close.size > 4096 + 1000 and int(g.order[bp]) == 10
    g.step(LONER, 0, 60000, route, form=(30, 256))
    g.close()


@pytest.fixture(scope="module", params=["sparse", "dense"])
def slow_world(request, oracle):
    """16-bit k = 9 under cfg5's `--feat slow` model at --id 0.6: a sparse set (the rank and divergence routes close_list switches on) and a
    dense one; 24 sequences of 1 kb +- 120 in families of six, slot 1 a copy of slot 0, one sequence cut to 400 bases"""
    fam, _ = synth.families(909, 24, 1000, family=6, length_jitter=120)
    seqs = [fam[0], fam[0]] + fam[2:23] + [fam[23][:400]]
    w = World(oracle, seqs, 9, 16, "weights_cfg5_k9.txt", 0.6, len(seqs), copies=[(0, 1)], sparse=request.param == "sparse")
    yield w
    w.close()


def test_sparse_and_slow_windows_see_ties_too(slow_world, route):
    w = slow_world
    n = 14000
    order = np.random.default_rng(9).integers(0, w.n_slots, size=n).astype(np.uint32)
    p = Pair(w, order)
    a, b = 2047, 2047 + 4 * SMALL_TILE + 9
    p.kill([a, a + SMALL_TILE - 1, a + SMALL_TILE])
    # (query 23, 400 bases: every other sequence is outside its length window, and it is outside theirs)
    for q in (0, 7, 13, 23, 19):
        close, bp, _, _ = p.step(q, a, b, route, form=(5, 256))
        v = w.verdict(q)
        if bp >= 0:
            top = np.flatnonzero(v.scored & (v.sim == v.sim[order[bp]]))
            alive_before = np.concatenate([p.mdl.alive_positions(a, b), close])
            assert bp == alive_before[np.isin(order[alive_before], top)].min()
        p.kill(p.mdl.alive_positions(a, b)[:5])
    p.step(1, 0, n, route, form=(7, 256))
    p.step(8, 0, 4096, route, form=(1, 1024))
    p.counts((a, b))
    p.close()
