"""The numpy restatement of msc_hist_canonical_batch that the canonical tests share: the rc permutation from the digit rule, the clamped sum and the
record's 1-mers. Nothing here calls the library."""
import numpy as np

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc_string(s):
    return s.translate(_COMP)[::-1]


def rc_perm(k):
    """perm[b] = rc(b): the bin whose digit of weight 4^j is 3 - (the digit of weight 4^(k-1-j) of b); A = 0, C = 1, G = 2, T = 3, first base most significant"""
    b = np.arange(4 ** k, dtype=np.int64)
    out = np.zeros_like(b)
    for j in range(k):
        digit = (b // 4 ** (k - 1 - j)) % 4          # the digit of weight 4^(k-1-j)
        out += (3 - digit) * 4 ** j
    return out


def palindromes(k):
    p = rc_perm(k)
    return np.flatnonzero(p == np.arange(p.size))


def canon(bins, k):
    """(clamp(D[b] + D[rc(b)] - 1, 0, max(T)) in D's type, whether some exact sum was past max(T))"""
    bins = np.asarray(bins)
    p = rc_perm(k)
    tmax = np.iinfo(bins.dtype).max
    if bins.dtype.itemsize < 8:
        exact = bins.astype(np.int64) + bins.astype(np.int64)[p] - 1
        return np.clip(exact, 0, tmax).astype(bins.dtype), bool((exact > tmax).any())
    a = bins.astype(np.uint64)
    s = a + a[p]                                      # wraps: a carry is s < a
    carry = s < a
    out = np.where(carry, np.uint64(tmax), np.where(s == 0, np.uint64(0), s - np.uint64(1))).astype(np.uint64)
    return out, bool((carry & (s != 0)).any())        # (carry with s == 0: the exact sum is 2^64 - 1, which fits)


def one_mers(om):
    """one_mers'[i] = one_mers[i] + one_mers[3 - i] - 1, in 64-bit words"""
    om = np.asarray(om, dtype=np.uint64)
    return om + om[::-1] - np.uint64(1)
