"""Helper run as a subprocess by test_gpu_build_routes.py (the library reads MSC_NO_LDS_BUILD, MSC_NO_SORT_DENSE_BUILD and
MSC_NO_SORT_BUILD once per process): every histogram builder msc_hist_build_packed can pick -- k_build_lds, k_build_sort (four LDS
classes), k_fill + k_count + k_finalize + k_prefix, k_sparse_build_sort, dense scratch + k_sparse_count / k_sparse_write -- against a
reference that does not go through the library, at the shapes where a builder goes wrong: every LDS class boundary, saturation of u8 /
u16 bins, every alignment of a segment in the packed 2-bit stream, empty records, rebuilt slots, long lists.

The reference: segments and effective length from the oracle's encoder (oracle_py.encode); k-mer indices (first base most significant)
computed in numpy over those segments, np.unique for the counts, pseudocount 1, clamp at max(T); for k <= 9 the oracle's own histogram
(oracle_py.hist) must equal the numpy bins. Read back per slot, through HistogramSet.device_view() + Context.memcpy_to_host: the 128-byte
MscSlotScalars record field by field, the S tile prefixes behind it, the raw tile-permuted slot (msc_layout.h restated here), and
download(); for sparse sets the byte range pack() writes (msc_shard.hip): scalar record, 16 + 1 sub-range offsets, (bin, value) list, cum.
Every integer is exact. stddev is held to sqrt((sum_sq - sum^2 / N) / N) in np.longdouble within the relative bound
8 * 2^-53 * (sum_sq + sum^2 / N) / (sum_sq - sum^2 / N) (at least 4 * 2^-53): the kernels evaluate (b - 2 aq a + N aq^2) / N with
aq = a / N in FP64; the error of aq cancels to first order between the two products, the three roundings of the products and the two of the
sums are each relative to a term of at most b + a^2 / N, fused multiply-adds drop some of them, and the division and the square root
add less than two more units to a result whose relative error the square root has halved. A variance that is exactly 0 must give 0.

Every build asserts the builder msc_hist_set_build_info names against the rule of msc_api.hip (expect_builder) and, on a fresh set, the
set's bounds against the true maxima. Arrays go to <out_dir>/<case>.<what>.npy, the builder names to routes.json; the test compares both
across variants.

usage: build_route_check.py OUT_DIR [ORACLE_CACHE_DIR]
The reference depends on the inputs alone; with a cache directory, the first run stores it there and later runs read it."""
import json
import os
import pickle
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from meshclust2_amd import api  # noqa: E402
from meshclust2_amd._capi import MscError  # noqa: E402
from oracle import oracle_py  # noqa: E402

ENV = os.environ
NO_LDS, NO_SORT_DENSE, NO_SORT_SPARSE = "MSC_NO_LDS_BUILD" in ENV, "MSC_NO_SORT_DENSE_BUILD" in ENV, "MSC_NO_SORT_BUILD" in ENV
SORT_MAX = 32768                # k-mers per sequence the sort builders take (hist_build.hip kSortMaxKeys, msc_api.hip build_sparse_sort)
SUB = 16                        # index sub-ranges of a sparse list (msc_internal.h MSC_SPARSE_SUB)
REC_WORDS = 16                  # MscSlotScalars (msc_layout.h): 128 bytes
MAG, LENGTH, SUM, SUM_SQ, MAX_COUNT, ONE_MERS, STDDEV, OVERFLOW, ID, N_KMERS = 0, 1, 2, 3, 4, 5, 9, 10, 11, 12
PACK_SPARSE = 0x5332            # msc_shard.hip: kind of a packed sparse slot
U = 2.0 ** -53
DENSE_A = [(1, 16), (2, 32), (3, 8), (4, 16), (5, 16), (6, 64), (7, 8), (7, 32), (7, 64), (8, 8), (8, 16), (9, 32), (10, 8)]
SPARSE_A = [(8, 8), (9, 32), (11, 8), (13, 64)]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def up16(v):
    return (v + 15) & ~15


def rnd(n, seed):
    """n random unambiguous bases"""
    return ACGT[np.random.RandomState(seed).randint(0, 4, n)].tobytes()


class Layout:
    """msc_make_layout / msc_phys_index / msc_scalar_stride (msc_layout.h)"""

    def __init__(self, k, bits):
        self.k, self.bits, self.esz = k, bits, bits // 8
        self.E = 16 // self.esz
        self.nbins = 4 ** k
        hist_bytes = self.nbins * self.esz
        self.LPT = 4 if hist_bytes >= 4096 else 2 if hist_bytes >= 2048 else 1
        self.R = self.LPT * self.E
        self.tile_bins = 64 * self.R
        self.S = -(-self.nbins // self.tile_bins)
        self.padded = self.S * self.tile_bins
        self.slot_bytes = self.padded * self.esz
        self.stride = (128 + 8 * self.S + 127) // 128 * 128
        self.tmax = 2 ** bits - 1
        self._perm = None

    def perm(self):
        """physical element index of every logical bin"""
        if self._perm is None:
            b = np.arange(self.nbins, dtype=np.int64)
            tile, e = b // self.tile_bins, b % self.tile_bins
            lane, r = e // self.R, e % self.R
            t, j = r // self.E, r % self.E
            self._perm = tile * self.tile_bins + t * (64 * self.E) + lane * self.E + j
        return self._perm


_LAYOUTS = {}


def layout(k, bits):
    if (k, bits) not in _LAYOUTS:
        _LAYOUTS[(k, bits)] = Layout(k, bits)
    return _LAYOUTS[(k, bits)]


def expect_builder(L, sparse, kmers, grouped=True):
    """the builder msc_hist_build_packed must pick under this process's switches (msc_api.hip: use_lds / use_sort, build_sparse_sort)"""
    longest = max(kmers) if len(kmers) else 0
    if sparse:
        if not NO_SORT_SPARSE and grouped and longest <= SORT_MAX:
            return "k_sparse_build_sort"
        return expect_builder(L, False, kmers, grouped) + "+k_sparse_write"
    if L.nbins <= 16384 and L.S <= 16 and grouped and not NO_LDS:
        return "k_build_lds"
    if L.LPT == 4 and L.S >= 16 and L.S % 4 == 0 and grouped and not NO_SORT_DENSE and longest <= SORT_MAX:
        return "k_build_sort"
    return "k_count"


# ------------------------------------------------------------------------------------------------------------------ the reference
def seq_ref(codes, segs, k, eff=None):
    """codes: uint8 array, 0..3 inside the inclusive segments -> what a slot must hold, as sorted distinct k-mer indices + occurrences"""
    parts, ones = [], np.ones(4, dtype=np.int64)
    for s, e in segs:
        c = codes[s:e + 1].astype(np.int64)
        assert c.size == e - s + 1 and (c < 4).all(), (s, e)
        ones += np.bincount(c, minlength=4)
        n = c.size - k + 1
        if n <= 0:
            continue
        idx = np.zeros(n, dtype=np.int64)
        for j in range(k):
            idx = idx * 4 + c[j:j + n]
        parts.append(idx)
    allk = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    keys, occ = np.unique(allk, return_counts=True)
    return dict(keys=keys.astype(np.int64), occ=occ.astype(np.int64), n_kmers=int(allk.size), one_mers=[int(x) for x in ones],
                eff=int(sum(e - s + 1 for s, e in segs)) if eff is None else int(eff))


def encode_ref(seq, k, bits):
    """one sequence through the oracle's encoder; for k <= 9 the oracle's histogram must be the numpy one"""
    codes, segs, eff = oracle_py.encode(seq)
    r = seq_ref(np.frombuffer(codes, dtype=np.uint8), segs, k, eff)
    r["segs"], r["codes"] = [(int(s), int(e)) for s, e in segs], codes
    if k <= 9:
        L = layout(k, bits)
        sl = SlotRef(L, r)
        oh = oracle_py.hist(seq, k, bits)
        try:
            assert np.array_equal(oh.array(), sl.bins()), "numpy bins differ from the oracle's"
            assert (oh.mag, oh.length, list(oh.one_mers), int(oh.overflow != 0)) == (sl.sum, r["eff"], r["one_mers"], sl.overflow), (oh.mag, oh.length, sl.sum)
        finally:
            oracle_py.lib().orc_hist_free(oh)
    return r


class SlotRef:
    """a slot of layout L holding the k-mers of r: bins, scalar record, tile prefixes, sparse list"""

    def __init__(self, L, r):
        self.L, self.r = L, r
        self.keys = r["keys"]
        v = 1 + r["occ"]
        self.overflow = int(bool((v > L.tmax).any())) if L.bits < 64 else 0
        self.vals = np.minimum(v, L.tmax) if L.bits < 64 else v
        ex = self.vals - 1
        self.sum = L.nbins + int(ex.sum())
        self.sum_sq = L.nbins + int((self.vals * self.vals - 1).sum())
        self.max_count = int(self.vals.max()) if self.vals.size else 1
        self.nnz = int(self.keys.size)
        cumex = np.cumsum(ex)
        self.cum = cumex.astype(np.uint32)
        bounds = np.arange(L.S, dtype=np.int64) * L.tile_bins          # prefix[t]: the stored bins of logical index < t * tile_bins
        pos = np.searchsorted(self.keys, bounds, side="left")
        before = np.where(pos > 0, cumex[np.maximum(pos, 1) - 1] if cumex.size else 0, 0)
        self.prefix = (np.minimum(bounds, L.nbins) + before).astype(np.uint64)
        self.split = np.searchsorted(self.keys, np.arange(SUB + 1, dtype=np.int64) * (L.nbins // SUB), side="left").astype(np.uint32)

    def record(self):
        """the integer words of MscSlotScalars (the stddev word left 0)"""
        w = np.zeros(REC_WORDS, dtype=np.uint64)
        w[MAG], w[LENGTH], w[SUM], w[SUM_SQ], w[MAX_COUNT] = self.sum, self.r["eff"], self.sum, self.sum_sq, self.max_count
        w[ONE_MERS:ONE_MERS + 4] = self.r["one_mers"]
        w[OVERFLOW], w[ID], w[N_KMERS] = self.overflow, 0, self.r["n_kmers"]
        return w

    def stddev(self):
        """-> (value in extended precision, absolute tolerance)"""
        N, a, b = np.longdouble(self.L.nbins), np.longdouble(self.sum), np.longdouble(self.sum_sq)
        m = a * a / N
        if self.sum_sq * self.L.nbins == self.sum * self.sum:
            return 0.0, 0.0
        exp = np.sqrt((b - m) / N)
        rel = max(8 * U * float((b + m) / (b - m)), 4 * U)
        return float(exp), rel * float(exp)

    def bins(self):
        out = np.ones(self.L.nbins, dtype=api.NP_T[self.L.bits])
        out[self.keys] = self.vals
        return out

    def raw(self):
        """the slot as it lies in HBM: the bins through msc_phys_index, zero pads"""
        out = np.zeros(self.L.padded, dtype=api.NP_T[self.L.bits])
        out[self.L.perm()] = self.bins()
        return out.view(np.uint8)


def no_std(sparse, read):
    """a read of slots (Check.verify_* / read_*) with the stddev word of every record cleared"""
    if sparse:
        out = [img.copy() for img in read]
        for img in out:
            img[16 + 8 * STDDEV:16 + 8 * STDDEV + 8] = 0
        return out
    rec = read[0].copy()
    rec[:, STDDEV] = 0
    return rec, read[1]


def pack_stream(code_arrays, align):
    """2-bit stream of the sequences, each starting on a multiple of `align` bases (msc_hist_build: 4) -> (bytes, n_bases, starts)"""
    starts, at = [], 0
    for c in code_arrays:
        starts.append(at)
        at += -(-len(c) // align) * align
    n_bases = at
    flat = np.zeros(-(-n_bases // 4) * 4, dtype=np.uint8)
    for c, s in zip(code_arrays, starts):
        flat[s:s + len(c)] = np.asarray(c, dtype=np.uint8) & 3
    q = flat.reshape(-1, 4)
    return (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8), n_bases, starts


class Batch:
    """the arguments of build_packed for sequences given as (codes, segments) and their reference"""

    def __init__(self, k, items, align=4):
        self.packed, self.n_bases, starts = pack_stream([c for c, _ in items], align)
        self.refs = [seq_ref(np.asarray(c, dtype=np.uint8), segs, k) for c, segs in items]
        self.seg = [(i, st + s, st + e) for i, ((_, segs), st) in enumerate(zip(items, starts)) for s, e in segs]
        self.n = len(items)

    def args(self, first, order=None):
        seg = self.seg if order is None else [self.seg[i] for i in order]
        return (first, self.n, self.packed, self.n_bases, [s[0] for s in seg], [s[1] for s in seg], [s[2] for s in seg],
                [r["eff"] for r in self.refs], [x for r in self.refs for x in r["one_mers"]])


def codes_of(seq):
    """A/C/G/T -> 0..3, anything else -> 1 (what the encoder writes for an N inside a segment; outside segments never read)"""
    lut = np.ones(256, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    return lut[np.frombuffer(seq, dtype=np.uint8)]


# ------------------------------------------------------------------------------------------------------------------ the checker
class Check:
    def __init__(self, out_dir, cache):
        self.ctx = api.Context(0)
        self.out_dir, self.cache = out_dir, cache
        if cache:
            os.makedirs(cache, exist_ok=True)
        self.dumps, self.routes = {}, {}
        self.n_slots = 0

    def cached(self, key, fn):
        path = os.path.join(self.cache, key + ".pkl") if self.cache else None
        if path and os.path.exists(path):
            with open(path, "rb") as f:
                return pickle.load(f)
        val = fn()
        if path:
            with open(path + ".tmp", "wb") as f:
                pickle.dump(val, f)
            os.replace(path + ".tmp", path)
        return val

    def refs(self, key, seqs, k, bits):
        return self.cached("%s_k%d_u%d" % (key, k, bits), lambda: [encode_ref(s, k, bits) for s in seqs])

    def new_set(self, k, bits, capacity, sparse, entries=0):
        return api.HistogramSet(self.ctx, k, bits, capacity, sparse_entries=(entries + 64) if sparse else 0)

    # -------------------------------------------------------------------------------------------------------------- reading slots
    def read_dense(self, hs, L, first, n):
        """-> (records + prefixes [n, 16 + S] uint64, raw slots [n, slot_bytes] uint8)"""
        b, sb, s, ss = hs.device_view()
        assert (sb, ss) == (L.slot_bytes, L.stride), (sb, ss)
        rec = self.ctx.memcpy_to_host(s + first * ss, n * ss).reshape(n, ss)[:, :8 * (REC_WORDS + L.S)].copy().view(np.uint64)
        raw = self.ctx.memcpy_to_host(b + first * sb, n * sb).reshape(n, sb)
        return rec, raw

    def read_sparse(self, hs, slots):
        """-> the packed byte range of each slot (pads zero: the buffer is cleared first)"""
        sizes = [hs.packed_bytes(s) for s in slots]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        dev = self.ctx.device_malloc(int(offs[-1]))
        try:
            self.ctx.memcpy_to_device(dev, np.zeros(int(offs[-1]), dtype=np.uint8))
            hs.pack(slots, dev, offs[:-1])
            img = self.ctx.memcpy_to_host(dev, int(offs[-1]))
        finally:
            self.ctx.device_free(dev)
        return [img[int(offs[i]):int(offs[i + 1])].copy() for i in range(len(slots))]

    def hold_record(self, name, words, sl):
        """16 record words against the reference: integers exact, stddev within the derived bound -> (got, expected, tolerance)"""
        got = words[:REC_WORDS].copy()
        sd = float(got[STDDEV:STDDEV + 1].view(np.float64)[0])
        got[STDDEV] = 0
        exp = sl.record()
        assert np.array_equal(got, exp), (name, "record", got.tolist(), exp.tolist())
        e, tol = sl.stddev()
        assert abs(sd - e) <= tol, (name, "stddev", sd, e, tol)
        return sd, e, tol

    def verify_dense(self, name, hs, L, first, refs, dump=True):
        rec, raw = self.read_dense(hs, L, first, len(refs))
        std = np.zeros((len(refs), 3))
        for i, r in enumerate(refs):
            sl, tag = SlotRef(L, r), (name, first + i)
            std[i] = self.hold_record(tag, rec[i], sl)
            assert np.array_equal(rec[i, REC_WORDS:], sl.prefix), (tag, "prefixes", np.flatnonzero(rec[i, REC_WORDS:] != sl.prefix)[:8].tolist())
            assert np.array_equal(raw[i], sl.raw()), (tag, "raw slot")
            assert np.array_equal(hs.download(first + i), sl.bins()), (tag, "download")
            info = hs.info(first + i)
            assert (info["sum"], info["sum_sq"], info["max_count"], info["overflow"]) == (sl.sum, sl.sum_sq, sl.max_count, sl.overflow), tag
        self.n_slots += len(refs)
        if dump:
            self.dumps[name + ".rec"], self.dumps[name + ".std"], self.dumps[name + ".raw"] = no_std(False, (rec, raw))[0], std, raw
        return rec, raw

    def verify_sparse(self, name, hs, L, first, refs, dump=True):
        imgs = self.read_sparse(hs, list(range(first, first + len(refs))))
        std = np.zeros((len(refs), 3))
        for i, (img, r) in enumerate(zip(imgs, refs)):
            sl, tag, n = SlotRef(L, r), (name, first + i), int(r["keys"].size)
            head = img[:16]
            assert (int(head[:2].view(np.uint16)[0]), int(head[2]), int(head[3]), int(head[4:8].view(np.uint32)[0]), int(head[8:16].view(np.uint64)[0])) == \
                (PACK_SPARSE, L.k, L.bits, n, img.size), (tag, "head")
            assert img.size == 16 + 128 + 80 + up16(8 * n) + up16(4 * n), (tag, img.size, n)
            std[i] = self.hold_record(tag, img[16:144].view(np.uint64), sl)
            assert np.array_equal(img[144:144 + 4 * (SUB + 1)].view(np.uint32), sl.split), (tag, "sub-range table", img[144:212].view(np.uint32).tolist(), sl.split.tolist())
            ent = img[224:224 + 8 * n].view(np.uint32).reshape(n, 2)
            assert np.array_equal(ent[:, 0], sl.keys) and np.array_equal(ent[:, 1], sl.vals), (tag, "list")
            at = 224 + up16(8 * n)
            assert np.array_equal(img[at:at + 4 * n].view(np.uint32), sl.cum), (tag, "cum")
            assert hs.entries(first + i) == n, (tag, "entries")
            if L.k <= 10:
                assert np.array_equal(hs.download(first + i), sl.bins()), (tag, "download")
        self.n_slots += len(refs)
        if dump:
            self.dumps[name + ".pack"], self.dumps[name + ".std"] = np.concatenate(no_std(True, imgs)), std
        return imgs

    def verify(self, name, hs, L, sparse, first, refs, dump=True):
        return (self.verify_sparse if sparse else self.verify_dense)(name, hs, L, first, refs, dump)

    def true_bounds(self, L, sparse, refs):
        sl = [SlotRef(L, r) for r in refs]
        return (max(s.max_count for s in sl), max(s.sum for s in sl), max(s.nnz for s in sl) if sparse else 0)

    def route(self, name, hs, L, sparse, refs, grouped=True):
        builder = hs.build_info()[0]
        want = expect_builder(L, sparse, [r["n_kmers"] for r in refs], grouped)
        assert builder == want, (name, builder, want)
        self.routes[name] = builder
        return builder

    def build(self, name, k, bits, sparse, seqs, dump=True):
        """seqs into a fresh set through msc_hist_build: the builder's name, the bounds, every slot"""
        L = layout(k, bits)
        refs = self.refs(name, seqs, k, bits)
        hs = self.new_set(k, bits, len(seqs), sparse, sum(r["n_kmers"] for r in refs))
        hs.build(seqs)
        self.route(name, hs, L, sparse, refs)
        bounds = hs.build_info()[1:]
        assert bounds == self.true_bounds(L, sparse, refs), (name, bounds, self.true_bounds(L, sparse, refs))
        if dump:
            self.dumps[name + ".bounds"] = np.array(bounds, dtype=np.uint64)
        return hs, refs, self.verify(name, hs, L, sparse, 0, refs, dump)

    # -------------------------------------------------------------------------------------------------------------- cases
    def route_table(self):
        """A. every (k, bin type) whose builder a switch moves: histograms under one tile (k <= 3, padded), 2 KiB, 4 KiB, the 16-tile
        limit of the LDS builder on either side ((7, 32): 16 tiles, (7, 64): 32), and the sparse layouts from its smallest to k = 13"""
        seqs = [rnd(700, 11), rnd(64, 12) + b"N" * 12 + rnd(333, 13), b"AC" * 150, rnd(2500, 14)]
        for k, bits in DENSE_A:
            self.build("A_dense_k%d_u%d" % (k, bits), k, bits, False, seqs)
        for k, bits in SPARSE_A:
            self.build("A_sparse_k%d_u%d" % (k, bits), k, bits, True, seqs[:2] if k == 13 else seqs)

    def key_counts(self):
        """B. exactly 0, 1, 255 .. 32768 k-mers per sequence in one batch (every LDS class with P keys, P + 1 and P - 1; sparse also
        P = 64, 128 and 256); then the same batch and one sequence of 32769, which takes the whole batch to another builder and must leave
        every slot as it was"""
        counts = [0, 1, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 16384, 16385, 32768]
        for k, bits, sparse in ((8, 8, False), (9, 32, False), (9, 32, True)):
            cs = counts + ([63, 64, 65, 128, 129] if sparse else [])
            seqs = [rnd(n + k - 1, 200 + i) for i, n in enumerate(cs)]
            name = "B_%s_k%d_u%d" % ("sparse" if sparse else "dense", k, bits)
            hs, refs, got = self.build(name, k, bits, sparse, seqs)
            assert [r["n_kmers"] for r in refs] == cs, name
            hs2, refs2, got2 = self.build(name + "_32769", k, bits, sparse, seqs + [rnd(32769 + k - 1, 299)])
            assert refs2[-1]["n_kmers"] == 32769
            L = layout(k, bits)
            moved = expect_builder(L, sparse, cs) != expect_builder(L, sparse, cs + [32769])
            assert (self.routes[name] != self.routes[name + "_32769"]) == moved, (self.routes[name], self.routes[name + "_32769"])
            if not (NO_SORT_SPARSE if sparse else NO_SORT_DENSE):
                assert moved, name
            self.same(name + "_32769", sparse, got, got2[:len(cs)] if sparse else (got2[0][:len(cs)], got2[1][:len(cs)]), other_builder=True)

    def saturation(self):
        """C. u8 at k = 8: 253 / 254 / 255 occurrences (254, 255, and 255 with the overflow flag), saturated runs in the first, a
        middle and the last tile, alone and between random flanks, and 128 saturated bins at once (the whole of k_build_sort's s_sat);
        u16 at k = 8: 65534 occurrences (65535, no flag: the plain atomic of k_count) and 65535 (the compare-and-swap form), alone and
        beside a sequence that starts with the neighbouring bin of the same 32-bit word. The same into sparse sets."""
        k = 8
        units, seen = [], set()
        for x in range(4 ** 8):          # sixteen primitive 8-base units whose rotation sets are pairwise disjoint, spread over the index range
            u = bytes(b"ACGT"[(x >> (2 * (7 - j))) & 3] for j in range(8))
            rot = {u[i:] + u[:i] for i in range(8)}
            if len(rot) == 8 and not (rot & seen) and x % 4096 >= 1000 and len(units) == x // 4096:
                units.append(u)
                seen |= rot
        assert len(units) == 16, len(units)
        sat128 = b"".join(u * 255 + u[:7] for u in units)
        assert len(sat128) == 32752
        u8 = [b"A" * (253 + 7), b"A" * (254 + 7), b"A" * (255 + 7), b"T" * (255 + 7), b"C" * 300,
              rnd(200, 31) + b"C" + b"G" * (255 + 7) + b"C" + rnd(200, 32), sat128]
        for sparse in (False, True):
            name = "C_%s_u8" % ("sparse" if sparse else "dense")
            hs, refs, _ = self.build(name, k, 8, sparse, u8)
            sl = [SlotRef(layout(k, 8), r) for r in refs]
            assert [(s.max_count, s.overflow) for s in sl[:3]] == [(254, 0), (255, 0), (255, 1)], name
            assert refs[6]["n_kmers"] == 32745 and int((refs[6]["occ"] >= 255).sum()) == 128, (refs[6]["n_kmers"], int((refs[6]["occ"] >= 255).sum()))
            tiles = {int(t) for t in refs[6]["keys"][refs[6]["occ"] >= 255] // layout(k, 8).tile_bins}
            assert len(tiles) >= 8, tiles                      # (tiles before, at and after saturated runs)
        near = b"AAAAAAAC" + rnd(492, 33)
        batches = {"65534": [b"A" * 65541], "65535": [b"A" * 65542], "both": [b"A" * 65541, b"A" * 65542, near], "plain": [near, b"A" * 65541]}
        for sparse in (False, True):
            for tag, seqs in batches.items():
                name = "C_%s_u16_%s" % ("sparse" if sparse else "dense", tag)
                hs, refs, _ = self.build(name, k, 16, sparse, seqs)
                sl = {len(s): SlotRef(layout(k, 16), r) for s, r in zip(seqs, refs)}
                for n, want in ((65541, (65535, 0)), (65542, (65535, 1)), (500, None)):
                    if n in sl and want:
                        assert (sl[n].max_count, sl[n].overflow) == want, (name, n)
                if 500 in sl:
                    assert sl[500].keys[0] == 1, name

    def alignment(self):
        """D. segments at every offset of a 16-base word of the packed stream, the last k-mer on the stream's last base, records
        without k-mers, an ungrouped segment list, the stream in device memory"""
        for k, bits, sparse in ((5, 16, False), (8, 8, False), (8, 8, True)):
            L, tag = layout(k, bits), "D_%s_k%d" % ("sparse" if sparse else "dense", k)
            # a 16-base lead, 0..15 N, a run of k - 1, k, k + 1 or 40 bases: as the encoder segments them (short runs joined or dropped) ...
            seqs = [rnd(16, 400 + j) + b"N" * j + rnd(r, 420 + j) for r in (k - 1, k, k + 1, 40) for j in range(16)]
            self.build(tag + "_encoded", k, bits, sparse, seqs)
            # ... and with the lead and the run as two segments of their own (build_packed takes any segment list)
            items = [(codes_of(s), [(0, 15), (16 + j, 16 + j + r - 1)]) for s, (r, j) in zip(seqs, [(r, j) for r in (k - 1, k, k + 1, 40) for j in range(16)])]
            bt = Batch(k, items, align=16)
            for i in range(4):
                assert {s[1] % 16 for s in bt.seg[1::2][16 * i:16 * i + 16]} == set(range(16)), tag
            hs = self.new_set(k, bits, bt.n, sparse, sum(r["n_kmers"] for r in bt.refs))
            hs.build_packed(*bt.args(0))
            self.route(tag + "_runs", hs, L, sparse, bt.refs)
            self.verify(tag + "_runs", hs, L, sparse, 0, bt.refs)
            # the last k-mer ends on the last base of the stream, for every n_bases mod 16 (sequences packed without filler bases)
            hs = self.new_set(k, bits, 2, sparse, 16 * 80)
            for r in range(16):
                a, b = rnd(37, 440 + r), rnd(27 + r, 460 + r)
                bt = Batch(k, [(codes_of(a), [(0, 36)]), (codes_of(b), [(0, 26 + r)])], align=1)
                assert bt.n_bases % 16 == r and bt.seg[-1][2] == bt.n_bases - 1, tag
                hs.build_packed(*bt.args(0))
                self.route("%s_end%d" % (tag, r), hs, L, sparse, bt.refs)
                self.verify("%s_end%d" % (tag, r), hs, L, sparse, 0, bt.refs)
            # records without a k-mer (empty, N only, shorter than k) at the first, a middle and the last place
            sp = [b"", b"N" * 30, b"ACGT"[:k - 1] if k <= 5 else b"ACGTACG"]
            for i in range(3):
                batch = [sp[i], rnd(120, 480 + i), sp[(i + 1) % 3], rnd(33, 490 + i), sp[(i + 2) % 3]]
                _, refs, _ = self.build("%s_none%d" % (tag, i), k, bits, sparse, batch)
                assert [r["n_kmers"] for r in refs[::2]] == [0, 0, 0], tag
            # two sequences of two and three segments: grouped through msc_hist_build, grouped and interleaved through build_packed,
            # and grouped from a stream in device memory
            two = [rnd(40, 501) + b"N" * 12 + rnd(50, 502), rnd(30, 503) + b"N" * 15 + rnd(45, 504) + b"N" * 11 + rnd(25, 505)]
            hs0, refs, base = self.build(tag + "_two", k, bits, sparse, two)
            assert [len(r["segs"]) for r in refs] == [2, 3], tag
            bt = Batch(k, [(codes_of(s), r["segs"]) for s, r in zip(two, refs)])
            for r0, r1 in zip(refs, bt.refs):
                assert np.array_equal(r0["keys"], r1["keys"]) and np.array_equal(r0["occ"], r1["occ"]) and (r0["eff"], r0["one_mers"]) == (r1["eff"], r1["one_mers"])
            hs = self.new_set(k, bits, 2, sparse, 400)
            hs.build_packed(*bt.args(0))
            self.route(tag + "_two_packed", hs, L, sparse, refs)
            self.same(tag + "_two_packed", sparse, base, self.verify(tag + "_two_packed", hs, L, sparse, 0, refs, dump=False))
            dev = self.ctx.device_malloc(bt.packed.size)
            try:
                self.ctx.memcpy_to_device(dev, bt.packed)
                hs = self.new_set(k, bits, 2, sparse, 400)
                a = bt.args(0)
                hs.build_packed_dev(a[0], a[1], dev, *a[3:])
                self.route(tag + "_two_dev", hs, L, sparse, refs)
                self.same(tag + "_two_dev", sparse, base, self.verify(tag + "_two_dev", hs, L, sparse, 0, refs, dump=False))
            finally:
                self.ctx.device_free(dev)
            order = [0, 2, 1, 3, 4]                                  # segments of sequence 0, 1, 0, 1, 1
            hs = self.new_set(k, bits, 2, sparse, 400)
            if not sparse:
                hs.build_packed(*bt.args(0, order))
                assert self.route(tag + "_two_ungrouped", hs, L, sparse, refs, grouped=False) == "k_count", tag
                self.same(tag + "_two_ungrouped", sparse, base, self.verify(tag + "_two_ungrouped", hs, L, sparse, 0, refs, dump=False), other_builder=True)
            else:                                                    # a sparse set refuses it and stays as it was
                hs.build_packed(*bt.args(0))
                before, info = self.read_sparse(hs, [0, 1]), hs.build_info()
                try:
                    hs.build_packed(*bt.args(0, order))
                    raise AssertionError("%s: a sparse set took an ungrouped segment list" % tag)
                except MscError as e:
                    assert e.code == -1, e                         # MSC_ERR_INVALID_ARG
                self.same(tag + "_two_refused", True, before, self.read_sparse(hs, [0, 1]))
                assert hs.build_info() == info and [hs.entries(0), hs.entries(1)] == [r["keys"].size for r in refs], tag

    @staticmethod
    def same(name, sparse, a, b, other_builder=False):
        """two reads of the same slots (verify_* / read_*): bit for bit. Between two builders the stddev word is left out: each was held
        to the extended-precision value, and whether two kernels round the expression alike is up to the compiler's contraction"""
        if other_builder:
            a, b = no_std(sparse, a), no_std(sparse, b)
        if sparse:
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), name
        else:
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name

    def slots(self):
        """E. six sequences into slots 3..8 of twelve; slots 5..6 rebuilt with shorter, then with longer sequences: equal to a fresh build,
        every other slot untouched, the bounds the running maxima; dense: the reference bins through upload() give the builders' bytes"""
        first6 = [rnd(400, 601), rnd(900, 602), rnd(300, 603) + b"C" + b"A" * 60 + b"C" + rnd(300, 604), rnd(1500, 605), rnd(650, 606), rnd(1100, 607)]
        short2, long2 = [rnd(90, 611), rnd(45, 612)], [rnd(4000, 621) + b"G" * 90, rnd(2600, 622)]
        for k, bits, sparse in ((5, 16, False), (8, 8, False), (8, 8, True)):
            L, tag = layout(k, bits), "E_%s_k%d" % ("sparse" if sparse else "dense", k)
            hs = self.new_set(k, bits, 12, sparse, 40000)
            every = (lambda: self.read_sparse(hs, list(range(12)))) if sparse else (lambda: self.read_dense(hs, L, 0, 12))

            def kept(before, after, lo, hi):
                if sparse:
                    return all(np.array_equal(before[i], after[i]) for i in range(12) if not lo <= i < hi)
                return all(np.array_equal(x[i], y[i]) for x, y in zip(before, after) for i in range(12) if not lo <= i < hi)
            snap = every()
            refs = self.refs(tag, first6, k, bits)
            hs.build(first6, 3)
            self.route(tag, hs, L, sparse, refs)
            bounds = hs.build_info()[1:]
            assert bounds == self.true_bounds(L, sparse, refs), (tag, bounds)
            self.verify(tag, hs, L, sparse, 3, refs)
            now = every()
            assert kept(snap, now, 3, 9), tag
            for step, seqs in (("short", short2), ("long", long2)):
                snap = now
                fresh, r2, want = self.build("%s_%s_fresh" % (tag, step), k, bits, sparse, seqs, dump=False)
                hs.build(seqs, 5)
                self.route("%s_%s" % (tag, step), hs, L, sparse, r2)
                self.same("%s_%s" % (tag, step), sparse, want, self.verify("%s_%s" % (tag, step), hs, L, sparse, 5, r2))
                now = every()
                assert kept(snap, now, 5, 7), (tag, step)
                bounds = tuple(max(a, b) for a, b in zip(bounds, self.true_bounds(L, sparse, r2)))      # monotone: never below the slots' maxima
                assert hs.build_info()[1:] == bounds, (tag, step, hs.build_info(), bounds)
                self.dumps["%s_%s.bounds" % (tag, step)] = np.array(bounds, dtype=np.uint64)
            if not sparse:                                           # slots 3, 4 and 7 still hold first6[0], [1], [4]
                up = self.new_set(k, bits, 3, False)
                for i, (slot, r) in enumerate(((3, refs[0]), (4, refs[1]), (7, refs[4]))):
                    up.upload(i, SlotRef(L, r).bins(), r["eff"], r["one_mers"])
                    rec_u, raw_u = self.read_dense(up, L, i, 1)
                    rec_b, raw_b = now[0][slot].copy(), now[1][slot]
                    rec_u[0, N_KMERS] = rec_b[N_KMERS] = rec_u[0, ID] = rec_b[ID] = 0
                    assert np.array_equal(rec_u[0], rec_b) and np.array_equal(raw_u[0], raw_b), (tag, "upload", slot)

    def long_lists(self):
        """F. more than 32768 k-mers in one sparse list: the dense scratch slot (k = 13, u64: 512 MiB) and its compaction; with A's
        (9, 32) that is every bin type (k = 8, u16: 32769 k-mers, one past the sort builder's limit)"""
        for k, bits, n in ((11, 8, 40000), (13, 64, 33000), (8, 16, 32769 + 8 - 1)):
            name = "F_sparse_k%d_u%d" % (k, bits)
            hs, refs, _ = self.build(name, k, bits, True, [rnd(n, 700 + k)])
            assert refs[0]["n_kmers"] == n - k + 1 > SORT_MAX and self.routes[name] == "k_count+k_sparse_write", name
            hs.close()

    def save(self):
        for name, a in self.dumps.items():
            np.save(os.path.join(self.out_dir, name + ".npy"), a)
        with open(os.path.join(self.out_dir, "routes.json"), "w") as f:
            json.dump(self.routes, f, sort_keys=True, indent=0)


def main():
    out_dir = sys.argv[1]
    cache = sys.argv[2] if len(sys.argv) > 2 else None
    # STARTED before the first GPU call, DONE after the last check: a variant that left STARTED alone ran and failed, and is not run again
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "STARTED"), "w").close()
    t0 = time.time()
    chk = Check(out_dir, cache)
    print("context after %.1f s" % (time.time() - t0), flush=True)
    for case in (chk.route_table, chk.key_counts, chk.saturation, chk.alignment, chk.slots, chk.long_lists):
        t0 = time.time()
        case()
        print("ok %s (%.1f s)" % (case.__name__, time.time() - t0), flush=True)
    chk.save()
    open(os.path.join(out_dir, "DONE"), "w").close()
    print("BUILD_ROUTE_OK", chk.n_slots, "slots")


if __name__ == "__main__":
    main()
