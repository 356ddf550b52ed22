"""What the traceback tests share: a numpy restatement of msc_align_pairs_trace written from its definition in DESIGN.md 4.6h (not from the
kernel), a replay of a CIGAR that shares nothing with it, the loader of tests/golden/align_trace.npz and the text dump
tests/align_trace_schedule_check.cpp reads.

The forward pass is align_util.align_batch's -- anti-diagonals of the grid, one numpy statement per diagonal and batch -- and keeps, per
diagonal, the three decisions of every inner cell as a nibble: bits 0-1 the state that won the diagonal's maximum (0 match, 1 lower, 2 upper),
bit 2 lower continued, bit 3 upper continued. The walk then runs over the whole batch at once, one column of every open pair per step."""
import hashlib
import os

import numpy as np

import align_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "align_trace.npz")
DEFAULT = align_util.DEFAULT
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
MATCH, LOWER, UPPER = 0, 1, 2
LETTERS = "MIDNSHP=X"
SMALL = 40000          # cells of a fixture pair the CPU tests trace
EDGE_LA, EDGE_LB = (1, 3, 4, 5, 255, 256, 257, 513), (1, 2, 64, 300)


def trace_batch(firsts, seconds, params=DEFAULT):
    """-> (int64 [n, 3] score, length, matches; list of n uint32 arrays, the runs of each pair, run << 4 | op; bool [n] real)"""
    match, mismatch, gap_open, gap_cont = (int(v) for v in params)
    n = len(firsts)
    out = np.zeros((n, 3), dtype=np.int64)
    if n == 0:
        return out, [], np.zeros(0, dtype=bool)
    la = np.array([len(s) for s in firsts], dtype=np.int64)
    lb = np.array([len(s) for s in seconds], dtype=np.int64)
    assert la.min() >= 1 and lb.min() >= 1
    LA, LB = int(la.max()), int(lb.max())
    s1 = np.full((n, LA), 256, dtype=np.int16)          # (fillers that equal nothing; cells past a pair's own corner feed nothing it reads)
    s2 = np.full((n, LB), 257, dtype=np.int16)
    for p in range(n):
        s1[p, :la[p]] = np.frombuffer(bytes(firsts[p]), dtype=np.uint8)
        s2[p, :lb[p]] = np.frombuffer(bytes(seconds[p]), dtype=np.uint8)
    ninf = np.array([align_util.neg_inf(int(a), int(b), params) for a, b in zip(la, lb)], dtype=np.int32)
    gained = 1 if mismatch == match else 0
    every = np.arange(n)

    def fresh():
        return [np.zeros((n, LA + 1), dtype=np.uint32 if k & 1 else np.int32) for k in range(6)]

    def set_boundary(st, d):
        ms, mw, ls, lw, us, uw = st
        if d <= LB:          # column 0, row d
            ms[:, 0] = 0 if d == 0 else ninf
            ls[:, 0] = ninf
            us[:, 0] = -gap_open - d * gap_cont
            mw[:, 0] = lw[:, 0] = uw[:, 0] = d << 16
        if 1 <= d <= LA:     # row 0, column d
            ms[:, d] = ninf
            us[:, d] = ninf
            ls[:, d] = -gap_open - d * gap_cont
            mw[:, d] = lw[:, d] = uw[:, d] = d << 16

    # the nibbles of diagonal d's inner cells, columns lo(d) .. hi(d), at [d, pair, column - lo(d)]
    nibbles = np.zeros((LA + LB + 1, n, min(LA, LB)), dtype=np.uint8)
    start = np.zeros(n, dtype=np.int64)
    two, one, new = fresh(), fresh(), fresh()
    set_boundary(two, 0)
    set_boundary(one, 1)
    corner = la + lb
    for d in range(2, LA + LB + 1):
        lo, hi = max(1, d - LB), min(LA, d - 1)
        cur, left = slice(lo, hi + 1), slice(lo - 1, hi)
        a, b = one[0][:, cur] - (gap_open + gap_cont), one[4][:, cur] - gap_cont          # upper: from the cell above; opened from match wins a tie
        upper_cont = ~(a >= b)
        new[4][:, cur] = np.where(upper_cont, b, a)
        new[5][:, cur] = np.where(upper_cont, one[5][:, cur], one[1][:, cur]) + np.uint32(65536)
        a, b = one[0][:, left] - (gap_open + gap_cont), one[2][:, left] - gap_cont          # lower: from the cell to the left
        lower_cont = ~(a >= b)
        new[2][:, cur] = np.where(lower_cont, b, a)
        new[3][:, cur] = np.where(lower_cont, one[3][:, left], one[1][:, left]) + np.uint32(65536)
        dm, dl, du = two[0][:, left], two[2][:, left], two[4][:, left]          # match: the diagonal neighbour's three states; match, then lower, then upper
        best = np.maximum(np.maximum(dm, dl), du)
        won = np.where(best == dm, MATCH, np.where(best == dl, LOWER, UPPER))
        w = np.where(won == MATCH, two[1][:, left], np.where(won == LOWER, two[3][:, left], two[5][:, left]))
        rows = d - np.arange(lo, hi + 1)
        eq = s1[:, lo - 1:hi] == s2[:, rows - 1]
        new[0][:, cur] = best + np.where(eq, np.int32(match), np.int32(mismatch))
        new[1][:, cur] = w + np.where(eq, np.uint32(65537), np.uint32(65536 + gained))
        nibbles[d, :, :hi - lo + 1] = won | (lower_cont << 2) | (upper_cont << 3)
        set_boundary(new, d)
        for p in np.nonzero(corner == d)[0]:
            i = la[p]
            m, l, u = int(new[0][p, i]), int(new[2][p, i]), int(new[4][p, i])
            top = max(m, l, u)
            start[p] = MATCH if top == m else LOWER if top == l else UPPER
            wv = int(new[1][p, i] if top == m else new[3][p, i] if top == l else new[5][p, i])
            out[p] = (top, wv >> 16, wv & 0xffff)
        two, one, new = one, new, two
    # the walk, back from every pair's corner: one column of every pair still inside its grid per step
    i, j, st = la.copy(), lb.copy(), start.copy()
    cols = np.zeros((n, LA + LB), dtype=np.uint8)
    k = np.zeros(n, dtype=np.int64)
    inside = every
    while inside.size:
        ii, jj, ss = i[inside], j[inside], st[inside]
        nib = nibbles[ii + jj, inside, ii - np.maximum(1, ii + jj - LB)].astype(np.int64)
        eq = s1[inside, ii - 1] == s2[inside, jj - 1]
        cols[inside, k[inside]] = np.where(ss == MATCH, np.where(eq, OP_EQ, OP_X), np.where(ss == LOWER, OP_I, OP_D))
        k[inside] += 1
        st[inside] = np.where(ss == MATCH, nib & 3, np.where(ss == LOWER, np.where(nib & 4, LOWER, MATCH), np.where(nib & 8, UPPER, MATCH)))
        i[inside] -= ss != UPPER
        j[inside] -= ss != LOWER
        inside = np.nonzero((i > 0) & (j > 0))[0]
    # a real path ends on a boundary state that holds a true score: upper in column 0, lower in row 0, match at the corner
    real = ((i == 0) & (j == 0) & (st == MATCH)) | ((i == 0) & (j > 0) & (st == UPPER)) | ((j == 0) & (i > 0) & (st == LOWER))
    ops = []
    for p in range(n):
        back = np.concatenate([cols[p, :k[p]], np.full(i[p], OP_I, dtype=np.uint8), np.full(j[p], OP_D, dtype=np.uint8)])
        ops.append(encode(back[::-1]))
    return out, ops, real


def encode(columns):
    """the op of every column, in forward order -> the runs, run << 4 | op (uint32)"""
    columns = np.asarray(columns, dtype=np.uint32)
    first = np.concatenate([[0], np.flatnonzero(np.diff(columns.astype(np.int64))) + 1])
    runs = np.diff(np.concatenate([first, [columns.size]])).astype(np.uint32)
    return (runs << np.uint32(4)) | columns[first]


def edge_pairs(seed=5):
    """la x lb over the sizes at which the schedule changes (a lane's four columns, one stripe, two, three), related and unrelated"""
    rs = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    firsts, seconds = [], []
    for la in EDGE_LA:
        for lb in EDGE_LB:
            a = letters[rs.randint(0, 4, la)]
            firsts += [a.tobytes(), a.tobytes()]
            rel = np.resize(a, lb).copy()          # the first sequence cut or repeated to lb bytes, 5 % of them redrawn
            hit = rs.rand(lb) < 0.05
            rel[hit] = letters[rs.randint(0, 4, int(hit.sum()))]
            seconds += [rel.tobytes(), letters[rs.randint(0, 4, lb)].tobytes()]
    return firsts, seconds


def trace_many(firsts, seconds, params=DEFAULT, step=32, budget=192 << 20):
    """trace_batch over groups of pairs of similar size whose nibbles stay within `budget` bytes; results in the caller's order"""
    groups = {}
    for p in range(len(firsts)):
        groups.setdefault(((len(firsts[p]) - 1) // step, (len(seconds[p]) - 1) // step), []).append(p)
    out = np.zeros((len(firsts), 3), dtype=np.int64)
    ops = [None] * len(firsts)
    real = np.zeros(len(firsts), dtype=bool)
    for (ka, kb), idx in groups.items():
        a, b = (ka + 1) * step, (kb + 1) * step
        most = max(1, budget // ((a + b + 1) * min(a, b)))
        for at in range(0, len(idx), most):
            part = idx[at:at + most]
            t, o, r = trace_batch([firsts[p] for p in part], [seconds[p] for p in part], params)
            out[part], real[part] = t, r
            for p, runs in zip(part, o):
                ops[p] = runs
    return out, ops, real


def replay(ops, a, b, params=DEFAULT):
    """A CIGAR read against its two sequences, from the encoding alone: -> (affine score, columns, '=' columns). Raises AssertionError where
    the runs are not a CIGAR of (a, b): an unknown op, an empty run, adjacent runs of one op, a '=' over different bytes or an 'X' over equal
    ones, or bytes of either sequence left over."""
    match, mismatch, gap_open, gap_cont = (int(v) for v in params)
    a, b = np.frombuffer(bytes(a), dtype=np.uint8), np.frombuffer(bytes(b), dtype=np.uint8)
    i = j = score = columns = same = 0
    before = None
    for word in np.asarray(ops, dtype=np.uint32).tolist():
        run, op = word >> 4, word & 15
        assert run >= 1 and op in (OP_I, OP_D, OP_EQ, OP_X) and op != before, (run, op, before)
        before = op
        columns += run
        if op in (OP_EQ, OP_X):
            assert i + run <= a.size and j + run <= b.size
            equal = a[i:i + run] == b[j:j + run]
            assert equal.all() if op == OP_EQ else not equal.any(), (op, i, j, run)
            score += run * (match if op == OP_EQ else mismatch)
            same += run if op == OP_EQ else 0
            i, j = i + run, j + run
        else:
            score -= gap_open + run * gap_cont
            if op == OP_I:
                i += run
            else:
                j += run
    assert i == a.size and j == b.size, (i, a.size, j, b.size)
    return score, columns, same


def cigar_string(ops):
    return "".join("%d%s" % (int(w) >> 4, LETTERS[int(w) & 15]) for w in ops)


def digest(ops):
    return hashlib.sha256(np.asarray(ops, dtype="<u4").tobytes()).digest()


class Fixture:
    """tests/golden/align_trace.npz, for the pairs and parameter sets of align_pairs.npz: runs (uint32 [n_sets, n_pairs]), sha256 (uint8
    [n_sets, n_pairs, 32], of the runs' little-endian bytes) and real (bool [n_sets, n_pairs])"""

    def __init__(self, path=FIXTURE):
        z = np.load(path)
        self.runs, self.sha256, self.real = z["runs"], z["sha256"], z["real"].astype(bool)


def write_dump(path, seqs, params, first, second, ops):
    """align_util.write_dump's text form without results, then per parameter set and pair a line `n_runs word ...` (ops[set][pair])"""
    align_util.write_dump(path, seqs, params, first, second)
    with open(path, "a") as f:
        for s in range(len(params)):
            for runs in ops[s]:
                f.write(" ".join(str(int(v)) for v in [len(runs)] + list(runs)) + "\n")
