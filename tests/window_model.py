"""A model of msc_window (csrc/msc_window.hip) in numpy, no GPU: an order (position -> slot) and an alive flag per position.

What a get_close over a range returns follows from ONE verdict per distinct slot and query -- the CPU oracle's, taken on singletons -- and
from the alive flags alone:

    close positions   alive, in [first, end), their slot close; ascending. They die with the call.
    best position     the LOWEST alive position among the scored ones of maximal similarity (Trainer::get_close's strict '>' in
                      window order, cluster/Trainer.cpp:26-37,59), -1 where nothing is scored
    is_min            no close position
    alive count       what msc_window_alive says of the range before the call

so the model is the reference for the device's compaction (which positions reach the list, in whatever order), its kills, its tie rule
and the host's Fenwick counts. kill() refuses what msc_window_kill refuses and, like it, applies nothing of a refused call.

An arg-max against the oracle means something only where the oracle's similarities of two different slots are either the same bits or far
enough apart that the device's last bits cannot swap them: check_separation() holds a verdict to that."""
import numpy as np

SEPARATION = 1e-6          # relative; the device's similarity is held to the oracle's at 1e-8


class Verdict:
    """the oracle's word on every distinct slot for one query: close, scored (inside the length window) and the similarity"""

    def __init__(self, close, scored, sim):
        self.close = np.asarray(close, dtype=bool)
        self.scored = np.asarray(scored, dtype=bool)
        self.sim = np.asarray(sim, dtype=np.float64)
        assert self.close.shape == self.scored.shape == self.sim.shape and self.close.ndim == 1
        assert not np.any(self.close & ~self.scored), "a slot outside the length window is never close"


def oracle_verdict(oracle, pred, cutoff, q_hist, hists):
    """oracle.get_close on each histogram alone: close = its flag, scored = best_pos >= 0, sim = best_sim"""
    close, scored, sim = [], [], []
    for h in hists:
        flags, bp, bs, _ = oracle.get_close(pred, cutoff, q_hist, [h])
        close.append(bool(flags[0]))
        scored.append(bp >= 0)
        sim.append(bs)
    return Verdict(close, scored, sim)


def check_separation(v, copies=()):
    """any two scored slots' similarities are bit-equal or more than SEPARATION apart (relative); the slots of each group in `copies`
    (copies of one sequence) are bit-equal"""
    for group in copies:
        group = list(group)
        assert all(v.scored[s] == v.scored[group[0]] and v.sim[s] == v.sim[group[0]] and v.close[s] == v.close[group[0]] for s in group), group
    s = np.sort(v.sim[v.scored])
    if s.size < 2:
        return
    gap = np.diff(s)
    bad = (gap != 0) & (gap <= SEPARATION * np.maximum(np.abs(s[1:]), np.abs(s[:-1])))
    assert not bad.any(), ("similarities too near for an arg-max", s[1:][bad], gap[bad])


class WindowModel:
    def __init__(self, order):
        self.order = np.ascontiguousarray(order, dtype=np.uint32)
        assert self.order.ndim == 1
        self.n = self.order.size
        self.live = np.ones(self.n, dtype=bool)

    def _clip(self, first, end):
        end = min(int(end), self.n)
        first = int(first)
        return (first, end) if 0 <= first < end else (0, 0)

    def alive(self, first=0, end=None):
        a, b = self._clip(first, self.n if end is None else end)
        return int(np.count_nonzero(self.live[a:b]))

    def alive_positions(self, first=0, end=None):
        a, b = self._clip(first, self.n if end is None else end)
        return a + np.flatnonzero(self.live[a:b])

    def get_close(self, v, first, end):
        """-> (close positions, best position, best similarity, is_min, alive count before the call); the close positions die"""
        a, b = self._clip(first, end)
        live = self.live[a:b]
        slots = self.order[a:b]
        n_alive = int(np.count_nonzero(live))
        close = a + np.flatnonzero(live & v.close[slots])
        scored = live & v.scored[slots]
        best_pos, best_sim = -1, -1.0
        if scored.any():
            sims = np.where(scored, v.sim[slots], -np.inf)
            i = int(np.argmax(sims))          # (the first of equal maxima: the lowest position)
            best_pos, best_sim = a + i, float(sims[i])
        self.live[close] = False
        return close.astype(np.int64), best_pos, best_sim, close.size == 0, n_alive

    def kill(self, positions):
        """msc_window_kill: the whole call is refused (ValueError, nothing applied) for a position out of range, listed twice or dead"""
        p = np.asarray(positions, dtype=np.int64).reshape(-1)
        if p.size == 0:
            return
        if p.min() < 0 or p.max() >= self.n:
            raise ValueError("position out of range")
        if np.unique(p).size != p.size:
            raise ValueError("position listed twice")
        if not self.live[p].all():
            raise ValueError("position already dead")
        self.live[p] = False
