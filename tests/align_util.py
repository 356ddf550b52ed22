"""What the alignment tests share: a numpy restatement of the recurrence of msc_align_pairs, written from its definition in DESIGN.md 4.6e
(not from the kernel), the loader of tests/golden/align_pairs.npz and the text dump tests/align_schedule_check.cpp reads.

The restatement walks the anti-diagonals of the grid (cell (i, j): column i of the first sequence, row j of the second; diagonal d = i + j), so
one numpy statement covers every cell of a diagonal and, in align_batch, of a whole batch of pairs. Boundary row 0 and boundary column 0 are
entries of the same arrays. Every tie is written as the definition orders it."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "align_pairs.npz")
DEFAULT = (1, -1, 2, 1)


def neg_inf(la, lb, params):
    match, mismatch, gap_open, gap_cont = params
    v = 0
    if la != lb:
        v += -gap_open - abs(la - lb) * gap_cont
    return v + mismatch * min(la, lb) - 1


def align_batch(firsts, seconds, params=DEFAULT):
    """-> int64 [n, 3]: score, length, matches of every (firsts[p], seconds[p]); bytes objects, first = the definition's sequence 1"""
    match, mismatch, gap_open, gap_cont = (int(v) for v in params)
    n = len(firsts)
    out = np.zeros((n, 3), dtype=np.int64)
    if n == 0:
        return out
    la = np.array([len(s) for s in firsts], dtype=np.int64)
    lb = np.array([len(s) for s in seconds], dtype=np.int64)
    assert la.min() >= 1 and lb.min() >= 1
    LA, LB = int(la.max()), int(lb.max())
    s1 = np.full((n, LA), 256, dtype=np.int16)          # (fillers that equal nothing; cells past a pair's own corner feed nothing it reads)
    s2r = np.full((n, LB), 257, dtype=np.int16)         # the second sequences, reversed: row j sits at LB - j
    for p in range(n):
        s1[p, :la[p]] = np.frombuffer(bytes(firsts[p]), dtype=np.uint8)
        s2r[p, LB - lb[p]:] = np.frombuffer(bytes(seconds[p]), dtype=np.uint8)[::-1]
    ninf = np.array([neg_inf(int(a), int(b), params) for a, b in zip(la, lb)], dtype=np.int32)[:, None]
    gained = 1 if mismatch == match else 0          # the definition counts a column whose score is `match`

    def fresh():
        # score (int32) and length * 65536 + count (uint32) of match, lower, upper; index = column
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

    two, one, new = fresh(), fresh(), fresh()          # diagonals d - 2, d - 1 and d: three sets of arrays that take turns
    set_boundary(two, 0)
    set_boundary(one, 1)
    corner = la + lb
    for d in range(2, LA + LB + 1):
        lo, hi = max(1, d - LB), min(LA, d - 1)          # columns of the diagonal's inner cells
        cur, left = slice(lo, hi + 1), slice(lo - 1, hi)
        # upper: from the cell above (same column, diagonal d - 1); opened from match wins a tie
        a, b = one[0][:, cur] - (gap_open + gap_cont), one[4][:, cur] - gap_cont
        new[4][:, cur] = np.maximum(a, b)
        new[5][:, cur] = np.where(a >= b, one[1][:, cur], one[5][:, cur]) + np.uint32(65536)
        # lower: from the cell to the left (column - 1, diagonal d - 1)
        a, b = one[0][:, left] - (gap_open + gap_cont), one[2][:, left] - gap_cont
        new[2][:, cur] = np.maximum(a, b)
        new[3][:, cur] = np.where(a >= b, one[1][:, left], one[3][:, left]) + np.uint32(65536)
        # match: from the three states of the diagonal neighbour (column - 1, diagonal d - 2): match, then lower, then upper
        dm, dl, du = two[0][:, left], two[2][:, left], two[4][:, left]
        best = np.maximum(np.maximum(dm, dl), du)
        w = np.where(best == dm, two[1][:, left], np.where(best == dl, two[3][:, left], two[5][:, left]))
        eq = s1[:, lo - 1:hi] == s2r[:, LB - d + lo:LB - d + hi + 1]
        new[0][:, cur] = best + np.where(eq, np.int32(match), np.int32(mismatch))
        new[1][:, cur] = w + np.where(eq, np.uint32(65537), np.uint32(65536 + gained))
        set_boundary(new, d)
        for p in np.nonzero(corner == d)[0]:
            i = la[p]
            m, l, u = int(new[0][p, i]), int(new[2][p, i]), int(new[4][p, i])
            top = max(m, l, u)
            wv = int(new[1][p, i] if top == m else new[3][p, i] if top == l else new[5][p, i])
            out[p] = (top, wv >> 16, wv & 0xffff)
        two, one, new = one, new, two
    return out


def align(first, second, params=DEFAULT):
    return tuple(int(v) for v in align_batch([first], [second], params)[0])


def align_many(firsts, seconds, params=DEFAULT, step=32):
    """align_batch over groups of pairs of similar size (both lengths in the same bracket of `step`), so that a batch pads little; results in
    the caller's order"""
    groups = {}
    for p in range(len(firsts)):
        groups.setdefault(((len(firsts[p]) - 1) // step, (len(seconds[p]) - 1) // step), []).append(p)
    out = np.zeros((len(firsts), 3), dtype=np.int64)
    for idx in groups.values():
        out[idx] = align_batch([firsts[p] for p in idx], [seconds[p] for p in idx], params)
    return out


class Fixture:
    """tests/golden/align_pairs.npz: seqs (list of bytes), first / second (uint32 [n_pairs]), params (int [n_sets, 4]), result (int32 [n_sets, n_pairs, 3])"""

    def __init__(self, path=FIXTURE):
        z = np.load(path)
        self.text, self.offsets = z["text"], z["offsets"].astype(np.uint64)
        raw = self.text.tobytes()
        self.seqs = [raw[int(self.offsets[i]):int(self.offsets[i + 1])] for i in range(self.offsets.size - 1)]
        self.first, self.second = z["first"].astype(np.uint32), z["second"].astype(np.uint32)
        self.params, self.result = z["params"].astype(np.int64), z["result"].astype(np.int32)

    def cells(self):
        ln = np.array([len(s) for s in self.seqs], dtype=np.int64)
        return ln[self.first] * ln[self.second]


def write_dump(path, seqs, params, first, second, result=None):
    """The text form of a list of pairs: `n_seqs n_sets n_pairs`, a sequence per line, a parameter set per line, a pair per line and, where
    result ([n_sets, n_pairs, 3]) is given, `score length matches` per set and pair"""
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (len(seqs), len(params), len(first)))
        for s in seqs:
            f.write(s.decode("ascii") + "\n")
        for p in params:
            f.write("%d %d %d %d\n" % tuple(int(v) for v in p))
        for a, b in zip(first, second):
            f.write("%d %d\n" % (a, b))
        if result is not None:
            for s in range(len(params)):
                for r in result[s]:
                    f.write("%d %d %d\n" % tuple(int(v) for v in r))
