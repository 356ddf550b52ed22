"""What the banded-alignment tests share: a numpy restatement of the banded operator and of its certificate, written from their definition in
DESIGN.md 4.6f (not from the kernel), the parameter sets of the soundness test, the doubling sequence of msc_align_pairs_auto and the text dump
tests/align_band_schedule_check.cpp reads.

As align_util.align_batch, the restatement walks the anti-diagonals of the grid; a cell (i, j) outside its pair's band lo <= i - j <= hi,
boundary cells included, is set to (DEEP, 0) in all three states after the diagonal's update. Every pair of a batch has its own half-width."""
import numpy as np

import align_util

DEEP = -(1 << 30)
NO_BAND = 0xffffffff
DEFAULT_FIRST_BAND = 64

# the 16 sets under which a certificate is offered (the fixture's three, zero gap costs, mismatch > match, match = mismatch, negative and zero
# match) and three under which it is not (gap_open < 0, gap_continue < 0, max(match, mismatch) + 2 * gap_continue < 0)
OFFERED = [(1, -1, 2, 1), (2, -3, 5, 2), (1, -1, 0, 1), (1, -1, 0, 0), (1, -1, 2, 0), (-1, 1, 2, 1), (-1, 2, 1, 1), (1, 1, 2, 1), (0, 0, 1, 1), (-1, -1, 1, 1),
           (0, -1, 2, 1), (-1, -2, 1, 1), (-2, -3, 0, 1), (5, -4, 10, 1), (1, 2, 1, 1), (3, -2, 0, 3)]
REFUSED = [(1, -1, -1, 1), (1, -1, 2, -1), (-3, -4, 2, 1)]


def offered(params):
    match, mismatch, gap_open, gap_cont = params
    return gap_open >= 0 and gap_cont >= 0 and max(match, mismatch) + 2 * gap_cont >= 0


def certified(la, lb, w, params, score):
    match, mismatch, gap_open, gap_cont = (int(v) for v in params)
    mn, d, smax = min(la, lb), abs(la - lb), max(match, mismatch)
    if w >= mn:
        return True
    if not offered(params):
        return False
    ub = smax * (mn - w - 1) - 2 * gap_open - (2 * w + 2 + d) * gap_cont
    pb = align_util.neg_inf(la, lb, params) + max(smax * (mn - w - 1) - (w + 1) * gap_cont, -mn * gap_cont)
    return score > max(ub, pb)


def banded_batch(firsts, seconds, bands, params=align_util.DEFAULT):
    """-> int64 [n, 4]: score, length, matches of the banded operator at half-width bands[p] (a number serves every pair), and the certificate"""
    match, mismatch, gap_open, gap_cont = (int(v) for v in params)
    n = len(firsts)
    out = np.zeros((n, 4), dtype=np.int64)
    if n == 0:
        return out
    la = np.array([len(s) for s in firsts], dtype=np.int64)
    lb = np.array([len(s) for s in seconds], dtype=np.int64)
    w = np.minimum(np.broadcast_to(np.asarray(bands, dtype=np.int64), (n,)), 1 << 20)
    assert la.min() >= 1 and lb.min() >= 1 and w.min() >= 0
    lo = (np.minimum(0, la - lb) - w)[:, None]
    hi = (np.maximum(0, la - lb) + w)[:, None]
    LA, LB = int(la.max()), int(lb.max())
    s1 = np.full((n, LA), 256, dtype=np.int16)
    s2r = np.full((n, LB), 257, dtype=np.int16)          # the second sequences, reversed: row j sits at LB - j
    for p in range(n):
        s1[p, :la[p]] = np.frombuffer(bytes(firsts[p]), dtype=np.uint8)
        s2r[p, LB - lb[p]:] = np.frombuffer(bytes(seconds[p]), dtype=np.uint8)[::-1]
    ninf = np.array([align_util.neg_inf(int(a), int(b), params) for a, b in zip(la, lb)], dtype=np.int32)[:, None]
    gained = 1 if mismatch == match else 0
    column = np.arange(LA + 1, dtype=np.int64)[None, :]

    def fresh():
        return [np.zeros((n, LA + 1), dtype=np.uint32 if k & 1 else np.int32) for k in range(6)]

    def set_boundary(st, d):
        ms, mw, ls, lw, us, uw = st
        if d <= LB:          # column 0, row d
            ms[:, 0] = 0 if d == 0 else ninf[:, 0]
            ls[:, 0] = ninf[:, 0]
            us[:, 0] = -gap_open - d * gap_cont
            mw[:, 0] = lw[:, 0] = uw[:, 0] = d << 16
        if 1 <= d <= LA:     # row 0, column d
            ms[:, d] = ninf[:, 0]
            us[:, d] = ninf[:, 0]
            ls[:, d] = -gap_open - d * gap_cont
            mw[:, d] = lw[:, d] = uw[:, d] = d << 16

    def leave_the_band(st, d, first, last):
        """columns first .. last of diagonal d: cell (i, d - i) lies on diagonal 2 i - d of the grid"""
        on = 2 * column[:, first:last + 1] - d
        outside = (on < lo) | (on > hi)
        for k in range(6):
            st[k][:, first:last + 1][outside] = 0 if k & 1 else DEEP

    two, one, new = fresh(), fresh(), fresh()
    for st in (two, one, new):
        for k in (0, 2, 4):
            st[k][:] = DEEP
    set_boundary(two, 0)
    leave_the_band(two, 0, 0, 0)
    set_boundary(one, 1)
    leave_the_band(one, 1, 0, min(1, LA))
    corner = la + lb
    lo_all, hi_all = int(lo.min()), int(hi.max())
    for d in range(2, LA + LB + 1):
        # columns of the diagonal's inner cells: those that some pair of the batch has in band (2 i - d in lo .. hi) and two more on either
        # side, which leave_the_band resets -- the three sets of arrays take turns, and a set last held diagonal d - 3, whose in-band columns
        # reach at most two to the left of this one's. Everything else in a set is out of band and holds (DEEP, 0) already.
        first, last = max(1, d - LB, (d + lo_all + 1) // 2 - 2), min(LA, d - 1, (d + hi_all) // 2 + 2)
        if first > last:
            set_boundary(new, d)
            for c in (0, d):
                if d - LB <= c <= LA:
                    leave_the_band(new, d, c, c)
            two, one, new = one, new, two
            continue
        cur, left = slice(first, last + 1), slice(first - 1, last)
        a, b = one[0][:, cur] - (gap_open + gap_cont), one[4][:, cur] - gap_cont
        new[4][:, cur] = np.maximum(a, b)
        new[5][:, cur] = np.where(a >= b, one[1][:, cur], one[5][:, cur]) + np.uint32(65536)
        a, b = one[0][:, left] - (gap_open + gap_cont), one[2][:, left] - gap_cont
        new[2][:, cur] = np.maximum(a, b)
        new[3][:, cur] = np.where(a >= b, one[1][:, left], one[3][:, left]) + np.uint32(65536)
        dm, dl, du = two[0][:, left], two[2][:, left], two[4][:, left]
        best = np.maximum(np.maximum(dm, dl), du)
        wd = np.where(best == dm, two[1][:, left], np.where(best == dl, two[3][:, left], two[5][:, left]))
        eq = s1[:, first - 1:last] == s2r[:, LB - d + first:LB - d + last + 1]
        new[0][:, cur] = best + np.where(eq, np.int32(match), np.int32(mismatch))
        new[1][:, cur] = wd + np.where(eq, np.uint32(65537), np.uint32(65536 + gained))
        set_boundary(new, d)
        leave_the_band(new, d, first, last)
        for c in (0, d):
            if d - LB <= c <= LA:
                leave_the_band(new, d, c, c)
        for p in np.nonzero(corner == d)[0]:
            i = la[p]
            m, l, u = int(new[0][p, i]), int(new[2][p, i]), int(new[4][p, i])
            top = max(m, l, u)
            wv = int(new[1][p, i] if top == m else new[3][p, i] if top == l else new[5][p, i])
            out[p] = (top, wv >> 16, wv & 0xffff, certified(int(la[p]), int(lb[p]), int(w[p]), params, top))
        two, one, new = one, new, two
    return out


def banded(first, second, band, params=align_util.DEFAULT):
    return tuple(int(v) for v in banded_batch([first], [second], band, params)[0])


def banded_many(firsts, seconds, bands, params=align_util.DEFAULT, step=32):
    """banded_batch over groups of pairs of similar size, results in the caller's order"""
    bands = np.broadcast_to(np.asarray(bands, dtype=np.int64), (len(firsts),))
    groups = {}
    for p in range(len(firsts)):
        groups.setdefault(((len(firsts[p]) - 1) // step, (len(seconds[p]) - 1) // step), []).append(p)
    out = np.zeros((len(firsts), 4), dtype=np.int64)
    for idx in groups.values():
        out[idx] = banded_batch([firsts[p] for p in idx], [seconds[p] for p in idx], bands[idx], params)
    return out


# ------------------------------------------------------------------------------------- msc_align_pairs_auto's sequence of bands
def worth(la, lb, w):
    """a pair runs at half-width w only while a stripe's row window is at most half of the grid's rows"""
    diagonals = abs(la - lb) + 2 * w + 1
    cols = 1 if diagonals <= 128 else 2 if diagonals <= 512 else 4
    return w < min(la, lb) and 2 * min(lb, diagonals + 64 * cols - 1) <= lb


def auto_bands(firsts, seconds, params, first_band=0):
    """-> the band_used msc_align_pairs_auto reports: the first half-width of first_band, 2 first_band, ... that is still worth a banded run
    and at which the restatement certifies the pair, NO_BAND where the sequence ends before one does"""
    n = len(firsts)
    used = np.full(n, NO_BAND, dtype=np.int64)
    w = np.full(n, first_band or DEFAULT_FIRST_BAND, dtype=np.int64)
    todo = [p for p in range(n) if offered(params) and worth(len(firsts[p]), len(seconds[p]), int(w[p]))]
    while todo:
        r = banded_many([firsts[p] for p in todo], [seconds[p] for p in todo], w[todo], params, step=128)
        again = []
        for k, p in enumerate(todo):
            if r[k, 3]:
                used[p] = w[p]
                continue
            w[p] *= 2
            if worth(len(firsts[p]), len(seconds[p]), int(w[p])):
                again.append(p)
        todo = again
    return used


def write_dump(path, seqs, params, first, second, bands, result):
    """align_util.write_dump with a line of half-widths before the results and `score length matches certified` per parameter set, half-width
    and pair (result: [n_sets, n_bands, n_pairs, 4])"""
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (len(seqs), len(params), len(first), len(bands)))
        for s in seqs:
            f.write(s.decode("ascii") + "\n")
        for p in params:
            f.write("%d %d %d %d\n" % tuple(int(v) for v in p))
        for a, b in zip(first, second):
            f.write("%d %d\n" % (a, b))
        f.write(" ".join(str(int(b)) for b in bands) + "\n")
        for s in range(len(params)):
            for k in range(len(bands)):
                for r in result[s][k]:
                    f.write("%d %d %d %d\n" % tuple(int(v) for v in r))
