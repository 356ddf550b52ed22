"""The arithmetic behind msc_set_pairs_div_cells (bits_pair_div in pair_features.hip), replayed in numpy: the divergence sums of a pair from
the shared k-mers, three (count, count) cell counts and spot terms over the two lists of large bins equal the sum over all bins, and the
one-logarithm form of a term equals the reference's three-logarithm form. No device is needed."""
import numpy as np
import pytest

LN2 = np.log(2.0)


def term_reference(a, b, mag_a, mag_b):
    """predict/Feature.cpp:1235-1262, 988-1008 per bin: a, b = the counts of the call's first and second argument"""
    pp, pq = a / mag_a, b / mag_b
    avg = 0.5 * (pp + pq)
    return (pp - pq) * np.log(pp / pq), pp * np.log(pp / avg) + pq * np.log(pq / avg)


def term_kernel(p, q, log_p_over_q, x, y, lam):
    pp, pq = p * x, q * y
    lg, r = log_p_over_q + lam, pq / pp
    return (pp - pq) * lg, pp * ((1.0 + r) * np.log(2.0 / (1.0 + r)) - r * lg)


def from_cells(c, q):
    """c, q: the counts of the candidate (first argument) and the query, every bin >= 1"""
    nbins = c.size
    mag_c, mag_q = float(c.sum()), float(q.sum())
    x, y, lam = 1.0 / mag_c, 1.0 / mag_q, np.log(mag_q / mag_c)
    t11 = term_kernel(1.0, 1.0, 0.0, x, y, lam)
    list_c, list_q = np.nonzero(c >= 3)[0], np.nonzero(q >= 3)[0]          # sorted by bin
    p1 = int(np.sum((c >= 2) & (q >= 2)))
    acc = np.zeros(2)

    def spot(a, b):
        t = term_kernel(float(a), float(b), np.log(float(a) / float(b)), x, y, lam)
        acc[0] += t[0] - t11[0]
        acc[1] += t[1] - t11[1]

    b_ge2 = b_eq2 = a_eq2 = 0
    for i in list_c:
        b_ge2 += int(q[i] >= 2)
        b_eq2 += int(q[i] == 2)
        spot(c[i], q[i])
    in_c = set(list_c.tolist())
    for i in list_q:
        if int(i) in in_c:
            continue
        a_eq2 += int(c[i] >= 2)
        spot(c[i], q[i])
    d_c = int(c.sum()) - nbins - int(np.sum(c[list_c] - 2))
    d_q = int(q.sum()) - nbins - int(np.sum(q[list_q] - 2))
    n22 = p1 - b_ge2 - a_eq2
    n21 = (d_c - list_c.size) - n22 - a_eq2
    n12 = (d_q - list_q.size) - n22 - b_eq2
    assert n22 == int(np.sum((c == 2) & (q == 2))) and n21 == int(np.sum((c == 2) & (q == 1))) and n12 == int(np.sum((c == 1) & (q == 2)))
    f21 = term_kernel(2.0, 1.0, LN2, x, y, lam)
    f12 = term_kernel(1.0, 2.0, -LN2, x, y, lam)
    return [acc[s] + n22 * t11[s] + n21 * (f21[s] - t11[s]) + n12 * (f12[s] - t11[s]) + nbins * t11[s] for s in (0, 1)]


@pytest.mark.parametrize("seed", range(6))
def test_cells_and_spot_terms_give_the_sum_over_all_bins(seed):
    rng = np.random.default_rng(seed)
    nbins = 4096
    c, q = np.ones(nbins, dtype=np.int64), np.ones(nbins, dtype=np.int64)
    for h, n in ((c, 700 + 90 * seed), (q, 900 - 60 * seed)):
        np.add.at(h, rng.integers(0, nbins, size=n), 1)
    shared = rng.integers(0, nbins, size=12)
    c[shared[:8]] += rng.integers(2, 300, size=8)          # large in both, in one only, beside a bin of count 2
    q[shared[4:]] += rng.integers(2, 40, size=8)
    jd, js = term_reference(c.astype(float), q.astype(float), float(c.sum()), float(q.sum()))
    got = from_cells(c, q)
    # both sides add 4 096 FP64 terms of at most 0.3 to a result of about 1: summation error below 4 096 x 2^-53 x the sum of |terms| < 1e-12
    assert got[0] == pytest.approx(float(jd.sum()), rel=1e-12, abs=1e-15)
    assert got[1] == pytest.approx(float(js.sum()), rel=1e-12, abs=1e-15)


def test_equal_histograms_give_zero():
    c = np.ones(1024, dtype=np.int64)
    c[[3, 77, 500]] += [1, 5, 200]
    got = from_cells(c, c.copy())
    assert abs(got[0]) < 1e-15 and abs(got[1]) < 1e-15
