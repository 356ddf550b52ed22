"""Helper run as a subprocess by test_gpu_sparse_routes.py (the library reads the MSC_SPARSE_* switches once per process): the merge
kernels of sparse sets (sparse.hip) against the CPU oracle at the shapes where a merge-path kernel goes wrong -- chunk ends on ties,
empty and one-entry lists, very unequal lengths, every `parts`, the whole-list fit boundary, the count boundary of the narrow range --
and the operators built on them. Every 1 x M call asserts the kernel msc_last_kernel_info names. The raw statistics of a fixed list of
pairs go to <out_dir>/<case>.npy, which the test compares across variants.

usage: sparse_route_check.py OUT_DIR [ORACLE_CACHE_DIR]
The oracle's values depend on the inputs alone; with a cache directory, the first run stores them there and later runs read them."""
import json
import os
import pickle
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from golden_util import EXACT, FEATS, _divergence_longdouble, weights_text  # noqa: E402
from meshclust2_amd import api, synth  # noqa: E402
from oracle import oracle_py  # noqa: E402

os.environ["MSC_NO_RANKS_1XM"] = "1"          # (read on every call) k <= 9: the merge kernels, not the rank pass, score the lists
ENV = os.environ
DIV = ("jefferey_divergence", "jensen_shannon")
ALL_MASK = sum(1 << b for _, b in FEATS)
DIV_MASK = sum(1 << b for n, b in FEATS if n in DIV)
INT_MASK = ALL_MASK - DIV_MASK
COL = {n: i for i, (n, _) in enumerate(FEATS)}
INT_COLS = [i for i, (n, _) in enumerate(FEATS) if n not in DIV]
DIV_COLS = [COL[n] for n in DIV]
ORDERS = (api.ORDER_CAND_FIRST, api.ORDER_QUERY_FIRST)
MEAN_LISTS = (0, 2, 3, 4, 5, 7)      # operators(): the lists whose mean is also held to the oracle alone
NARROW_MAX_COUNT = 8191          # largest bin of the narrow range (msc_api_private.h): beyond it a pass is "wide"
KMP_CHUNK, KMP_CHUNK_WIDE = 512, 575          # merged entries per chunk of k_pair_sparse_mp (sparse.hip)


def mp_chunk(k):
    """the chunk the merge-path kernel walks at this k (sparse.hip mp_wide): 575 up to 4^11 bins, 512 above, or what MSC_SPARSE_MP_CHUNK forces"""
    force = int(ENV.get("MSC_SPARSE_MP_CHUNK", "0") or 0)
    return KMP_CHUNK_WIDE if force == 575 else KMP_CHUNK if force == 512 else KMP_CHUNK_WIDE if 4 ** k <= 1 << 22 else KMP_CHUNK


def mp_parts(m, entries, num_cus, div):
    """waves per pair a 1 x M launch of the merge-path kernel may use (sparse.hip msc_sparse_mp_parts)"""
    if "MSC_SPARSE_MP_NO_PARTS" in ENV or m == 0:
        return 1
    slots, chunks, parts = num_cus * (4 * 6 if div else 32), entries // KMP_CHUNK, 1
    if div:
        if m >= slots:
            return 1
        while parts < 16 and parts * 2 * 4 * 4 <= chunks and m * parts * 2 <= 2 * slots:
            parts *= 2
        return parts
    while parts < 16 and m * parts * 2 <= slots and parts * 2 * 2 <= chunks:
        parts *= 2
    return parts


def div_parts_of_pair(parts, total, chunk):
    """... of which a pair of `total` merged entries takes one per stretch of 4 granules of 4 chunks (k_pair_sparse_mp, DIV)"""
    n_chunks = -(-total // chunk)
    n_gran = -(-n_chunks // 4)
    return max(1, min(parts, n_gran // 4))


def mean_grouped(nbins, chunk_bins):
    """whether the sparse mean sweeps only the 64-byte lines the members touched (msc_api_private.h msc_sparse_groups_min_bins and the
    chunk rule of msc_api_score.hip / msc_api_batch.hip)"""
    if "MSC_SPARSE_MEAN_NO_GROUPS" in ENV:
        return False
    mk = max(5, min(16, int(ENV.get("MSC_SPARSE_MEAN_GROUPS_MIN_K", "9") or 9)))
    return nbins >= 4 ** mk and chunk_bins % 512 == 0


def distinct_prefix(seq, k, target):
    """the shortest prefix of seq with exactly `target` distinct k-mers (ACGT only: a sparse slot's entry count)"""
    seen = set()
    for i in range(len(seq) - k + 1):
        seen.add(seq[i:i + k])
        if len(seen) == target:
            return seq[:i + k]
    raise ValueError("sequence too short for %d distinct %d-mers" % (target, k))


def n_distinct(seq, k):
    return len({seq[i:i + k] for i in range(len(seq) - k + 1)})


def run_of(base, v, k):
    """a homopolymer run whose k-mer bin holds v (v - 1 occurrences + the pseudocount), fenced so that its neighbours do not extend it"""
    fence = b"C" if base == b"A" else b"A"
    return fence + base * (v + k - 2) + fence


class Oracle:
    """oracle_py values, read from / stored in the cache directory when there is one"""

    def __init__(self, cache):
        self.cache = cache
        if cache:
            os.makedirs(cache, exist_ok=True)

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

    def raw_table(self, key, seqs, k, dtype, pairs):
        """pairs (c, q, order) of sequence indices -> [len(pairs), 13]: the 11 raw statistics, then jefferey / jensen_shannon in extended
        precision. At most the histograms of the pairs in flight live on the host (a k = 11 u32 histogram is 16 MiB)."""
        def compute():
            last = {}
            for t, (c, q, _) in enumerate(pairs):
                last[c] = last[q] = t
            held, out = {}, np.zeros((len(pairs), len(FEATS) + 2))
            for t, (c, q, order) in enumerate(pairs):
                for s in (c, q):
                    if s not in held:
                        held[s] = oracle_py.hist(seqs[s], k, dtype)
                a, b = (held[c], held[q]) if order == api.ORDER_CAND_FIRST else (held[q], held[c])
                out[t, :len(FEATS)] = [oracle_py.raw_feature(1 << bit, a, b) for _, bit in FEATS]
                out[t, len(FEATS):] = [_divergence_longdouble(n, a, b) for n in DIV]
                for s in {c, q}:
                    if last[s] == t:
                        oracle_py.lib().orc_hist_free(held.pop(s))
            return out
        return self.cached(key, compute)


class Check:
    def __init__(self, out_dir, cache):
        self.ctx = api.Context(0)
        self.out_dir = out_dir
        self.oracle = Oracle(cache)
        self.dump = {}
        self.routes = {}          # which chunk / parts / mean sweep each case ran by the library's rules: routes.json, compared across variants
        self.n_calls = 0
        self.num_cus = int(re.search(r"(\d+) CUs", self.ctx.device_name()).group(1))

    # ---------------------------------------------------------------------------------------------------------- routes
    def expect(self, cset, q_nnz, max_count, div):
        """the kernel the switches of this process must select for a 1 x M pass (msc_api_score.hip pick_sparse_kernel + the wl rule)"""
        c_max = max(cset.entries(s) for s in range(cset.capacity))
        # (needs_wide, msc_api_score.hip, also calls a pass wide when a histogram's sum passes 2^31 - 1 or its excess times the layout's
        # R passes 2^32: no set here comes near either -- checked, so that the rule below stays the whole rule for these inputs)
        assert max(cset.info(s)["mag"] for s in range(cset.capacity)) < 1 << 26
        if max_count > NARROW_MAX_COUNT:
            return "k_pair_sparse"
        if "MSC_SPARSE_LDS" in ENV and ((q_nnz + 128) + 4 * (c_max + 128)) * 8 <= 96 * 1024:
            return "k_pair_sparse_lds"
        if "MSC_SPARSE_NO_MP" in ENV:
            return "k_pair_sparse"
        if not div and c_max and q_nnz + 4 * c_max + 10 <= 8192 and "MSC_SPARSE_NO_WL" not in ENV:
            return "k_pair_sparse_wl"
        return "k_pair_sparse_mp"

    def raw(self, cset, cands, qset, q, mask, order, want=None):
        r = api.pair_features_raw(self.ctx, cset, np.asarray(cands, dtype=np.uint32), qset, int(q), mask, order)
        self.n_calls += 1
        kern = self.ctx.last_kernel_info()[0]
        if want is None:
            mc = max(cset.info(s)["max_count"] for s in range(cset.capacity))
            mc = max(mc, qset.info(int(q))["max_count"])
            want = self.expect(cset, qset.entries(int(q)), mc, bool(mask & DIV_MASK))
        assert kern == want, (kern, want, mask)
        return r

    def score_pairs(self, name, cset, qset, cands, q, seqs, k, dtype, c_index, q_index, want=None):
        """all 11 statistics of cands x q in both argument orders, the integer form (INT_MASK) and the divergence form (DIV_MASK) equal
        to the columns of one call with both (ALL_MASK), held to the oracle; dumps the ALL_MASK values"""
        rows, ints, divs, kern = [], [], [], {}
        for order in ORDERS:
            rows.append(self.raw(cset, cands, qset, q, ALL_MASK, order, want))
            kern["all"] = self.ctx.last_kernel_info()[0]
            ints.append(self.raw(cset, cands, qset, q, INT_MASK, order, want))
            kern["int"] = self.ctx.last_kernel_info()[0]
            divs.append(self.raw(cset, cands, qset, q, DIV_MASK, order, want))
            kern["div"] = self.ctx.last_kernel_info()[0]
        pairs = [(c_index(c), q_index(q), order) for order in ORDERS for c in cands]
        exp = self.oracle.raw_table(name, seqs, k, dtype, pairs)
        got = np.concatenate(rows)
        alone = got.copy()
        alone[:, INT_COLS] = np.concatenate(ints)
        alone[:, DIV_COLS] = np.concatenate(divs)
        hold("%s (integer mask: %s)" % (name, kern["int"]), alone, exp, pairs, INT_COLS)
        hold("%s (divergence mask: %s)" % (name, kern["div"]), alone, exp, pairs, DIV_COLS)
        hold("%s (both: %s)" % (name, kern["all"]), got, exp, pairs)
        assert np.array_equal(got, alone, equal_nan=True), name          # a statistic does not depend on what else the call asked for
        self.dump[name] = got
        return got

    # ---------------------------------------------------------------------------------------------------------- cases
    def chunk_ends(self, k=11, dt=32, js=(1, 2, 3, 4), ds=(-2, -1, 0, 1, 2)):
        """a 3 kb query and near copies trimmed so that q_nnz + c_nnz = j * C + d (C = 512 and 575, j chunks past the query's own, d = -2..2):
        ties sit on every chunk end, the last chunk is one entry short of full, full, or spills over. At k = 11 (4^11 bins) the default
        chunk is 575, at k = 12 it is 512: each MSC_SPARSE_MP_CHUNK variant changes the chunk of one of the two."""
        name = "chunk_ends" if k == 11 else "k%d_chunk_ends" % k
        self.routes[name + "_chunk"] = mp_chunk(k)
        tmpl = synth.template(4601, 0, 3000)
        q = synth.to_ascii(tmpl)
        qn = n_distinct(q, k)
        seqs, targets = [q], []
        for C in (512, 575):
            j0 = qn // C
            for j in js:
                for d in ds:
                    t = (j0 + j) * C + d - qn
                    if t < 1:
                        continue
                    copy = synth.to_ascii(synth.member(4601, 0, len(seqs), tmpl, sub_rate=0.01, indel_rate=0.002))
                    seqs.append(distinct_prefix(copy, k, t))
                    targets.append(t)
        hs = api.HistogramSet(self.ctx, k, dt, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 4096)
        hs.build(seqs)
        assert hs.entries(0) == qn
        for i, t in enumerate(targets):
            assert hs.entries(i + 1) == t, (i, t)
        cands = np.arange(1, len(seqs), dtype=np.uint32)
        self.score_pairs(name, hs, hs, cands, 0, seqs, k, dt, int, int,
                         want=os.environ.get("MSC_TEST_EXPECT_KERNEL") or None)

    def degenerate(self):
        """k = 9: empty lists (shorter than k) as query, candidate and both; a one-entry list (a homopolymer of k + 5 bases: one bin of
        7); a candidate identical to the query (every entry ties); slot lists with repeats"""
        k, dt = 9, 16
        fam, _ = synth.families(4602, 5, 1000, family=5)
        seqs = [fam[0], fam[0], b"ACGTA", b"A" * (k + 5), fam[1], fam[2], fam[3], fam[4], b"ACGTACGT"]
        hs = api.HistogramSet(self.ctx, k, dt, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 4096)
        hs.build(seqs)
        assert hs.entries(2) == 0 and hs.entries(8) == 0 and hs.entries(3) == 1 and int(hs.download(3).max()) == 7
        assert hs.entries(0) == hs.entries(1) == n_distinct(fam[0], k)
        cands = np.array([1, 2, 3, 0, 2, 4, 5, 3, 6, 7, 1, 8, 8], dtype=np.uint32)
        for q in (0, 2, 3, 8):
            self.score_pairs("degenerate_q%d" % q, hs, hs, cands, q, seqs, k, dt, int, int)
        # every entry ties: the integer statistics of identical lists
        a = self.raw(hs, [1], hs, 0, ALL_MASK, api.ORDER_CAND_FIRST)[0]
        assert a[COL["manhattan"]] == 0.0 and a[COL["euclidean"]] == 0.0 and a[COL["emd"]] == 0.0, a

    def unequal_and_parts(self):
        """k = 11 / 80 kb (pairs of about 158 000 merged entries, long enough for 16 parts of either form): a one-entry list against
        the long lists and the reverse, in both orders; then windows of m = 1 .. 7000 (repeated slots) over the same pairs, whose rows
        must equal, bit for bit, the rows of every other m. By the library's rule the windows give the integer form 16, 8, 4, 2 and 1
        waves per pair and the divergence form 16, 8, 4, 2 and 1 (asserted below; MSC_SPARSE_MP_NO_PARTS: 1 throughout)."""
        k, dt = 11, 32
        fam, _ = synth.families(4603, 6, 80000, family=3)
        seqs = [b"C" * (k + 5)] + list(fam)
        n = len(seqs)
        hs = api.HistogramSet(self.ctx, k, dt, n, sparse_entries=sum(len(s) for s in seqs) + 4096)
        hs.build(seqs)
        assert hs.entries(0) == 1 and int(hs.download(0).max()) == 7
        self.score_pairs("unequal_q0", hs, hs, np.arange(1, n, dtype=np.uint32), 0, seqs, k, dt, int, int)
        self.score_pairs("unequal_q1", hs, hs, np.array([0, 2, 0, 3], dtype=np.uint32), 1, seqs, k, dt, int, int)
        base = np.arange(2, n, dtype=np.uint32)                      # 5 distinct 80 kb candidates against query 1
        pairs = [(int(c), 1, api.ORDER_CAND_FIRST) for c in base]
        exp = self.oracle.raw_table("parts", seqs, k, dt, pairs)
        entries = hs.entries(1) + max(hs.entries(s) for s in range(n))          # (the launch's bound: the query's list + the longest of the set)
        shortest = hs.entries(1) + min(hs.entries(int(c)) for c in base)
        ref, ran = {}, {}
        for mask in (INT_MASK, DIV_MASK):
            div = mask == DIV_MASK
            cols = DIV_COLS if div else INT_COLS
            for m in (1, 8, 64, 256, 1024, 2048, 4096, 5000, 7000):
                cands = np.resize(base, m)
                r = self.raw(hs, cands, hs, 1, mask, api.ORDER_CAND_FIRST)
                parts = mp_parts(m, entries, self.num_cus, div)
                if div:
                    parts = div_parts_of_pair(parts, shortest, mp_chunk(k))      # (every pair of the window reaches it: its shortest does)
                ran.setdefault("div" if div else "int", []).append(parts)
                wide = np.zeros((m, len(FEATS)))                  # (the columns of the statistics the mask asked for, in the 11-column layout)
                wide[:, cols] = r
                for i in range(min(m, len(base))):
                    hold("parts_m%d" % m, wide[i:i + 1], exp[i:i + 1], pairs[i:i + 1], cols)
                for i in range(m):
                    key = (mask, i % len(base))
                    if key in ref:
                        assert np.array_equal(r[i], ref[key], equal_nan=True), ("parts", m, i)
                    else:
                        ref[key] = r[i].copy()
            self.dump["parts_%s" % ("div" if div else "int")] = np.stack([ref[(mask, i)] for i in range(len(base))])
        self.routes["parts"] = ran
        if "MSC_SPARSE_MP_NO_PARTS" not in ENV and "MSC_SPARSE_NO_MP" not in ENV and self.num_cus == 256:
            assert set(ran["int"]) == set(ran["div"]) == {1, 2, 4, 8, 16}, ran
        # Q x M over the long lists: the queued merge-path passes == one 1 x M pass per query
        self.qxm(hs, np.array([1, 0, 2, 6], dtype=np.uint32), np.resize(np.arange(n, dtype=np.uint32), 300), "weights_k9_u32.txt", None)

    def wl_boundary(self):
        """k = 9: q_nnz + 4 c_max_nnz + 10 = 8192 (the whole-list kernel) against 8196 (one more entry in the longest candidate slot)
        and 8193 (one more in the query): the merge-path kernel"""
        k, dt = 9, 16
        cm, qn = 1500, 8182 - 4 * 1500
        fam, _ = synth.families(4604, 7, 3000, family=7)
        qseqs = [distinct_prefix(fam[0], k, qn), distinct_prefix(fam[0], k, qn + 1)]
        qs = api.HistogramSet(self.ctx, k, dt, 2, sparse_entries=8192)
        qs.build(qseqs)
        assert (qs.entries(0), qs.entries(1)) == (qn, qn + 1)
        for longest, name in ((cm, "wl_8192"), (cm + 1, "wl_8196")):
            seqs = [distinct_prefix(fam[1], k, longest)] + [distinct_prefix(f, k, 700 + 100 * i) for i, f in enumerate(fam[2:])]
            hs = api.HistogramSet(self.ctx, k, dt, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 4096)
            hs.build(seqs)
            assert max(hs.entries(s) for s in range(len(seqs))) == hs.entries(0) == longest
            allseqs = seqs + qseqs
            cands = np.array([0, 1, 2, 3, 4, 0, 5], dtype=np.uint32)
            for q in (0, 1):
                total = qs.entries(q) + 4 * longest + 10
                assert total in (8192, 8193, 8196, 8197)
                want_int = self.expect(hs, qs.entries(q), 255, False)
                if "MSC_SPARSE_LDS" not in ENV and "MSC_SPARSE_NO_MP" not in ENV:
                    assert want_int == ("k_pair_sparse_wl" if total == 8192 and "MSC_SPARSE_NO_WL" not in ENV else "k_pair_sparse_mp"), (total, want_int)
                self.score_pairs("%s_q%d" % (name, q), hs, qs, cands, q, allseqs, k, dt, int, lambda q_: len(seqs) + q_)
        # Q x M whose queries straddle the rule (the set's longest list: 1900 entries; 300 fits, 700 / 1000 / 1200 do not): the queued
        # passes take the whole-list kernel query by query, and the name says so
        seqs = [distinct_prefix(f, k, t) for f, t in zip(fam[1:], (1900, 300, 1000, 700, 1200))]
        hs = api.HistogramSet(self.ctx, k, dt, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 4096)
        hs.build(seqs)
        assert [hs.entries(i) for i in range(len(seqs))] == [1900, 300, 1000, 700, 1200]
        cands = np.array([0, 1, 2, 3, 4, 2, 1], dtype=np.uint32)
        self.qxm(hs, np.array([1, 2, 4], dtype=np.uint32), cands, "weights_k9_u32.txt", (seqs, k, dt), key="qxm_mixed")
        self.qxm(hs, np.array([1, 1], dtype=np.uint32), cands, "weights_k9_u32.txt", (seqs, k, dt), key="qxm_fits")

    def count_boundary(self):
        """k = 9: the largest bin from a homopolymer run -- u8 saturated at 255; u16 at 8191 (the narrow range: merge-path / whole-list
        kernels), 8192 and 46340 (the lane-per-sub-range kernel; from a difference of 46341 on, the reference squares u8 / u16 counts in
        a signed int that overflows, which is undefined); u32 at 65535; u64 at 65536 (a u32 count of 2^16 squares to 0 in the reference's
        32-bit products, which the GPU kernels do not reproduce)"""
        k = 9
        fam, _ = synth.families(4605, 4, 1000, family=4)
        for dt, v, top in ((8, 300, 255), (16, 8191, 8191), (16, 8192, 8192), (16, 46340, 46340), (32, 65535, 65535), (64, 65536, 65536)):
            mono = fam[1][:500] + run_of(b"A", v, k) + fam[1][500:]
            seqs = [fam[0], mono, fam[2], fam[3], fam[1]]
            hs = api.HistogramSet(self.ctx, k, dt, len(seqs), sparse_entries=sum(len(s) for s in seqs) + 4096)
            hs.build(seqs)
            assert int(hs.download(1).max()) == top, (dt, v)
            cands = np.array([0, 1, 2, 3, 4, 1], dtype=np.uint32)
            for q in (1, 0):
                self.score_pairs("count_u%d_%d_q%d" % (dt, v, q), hs, hs, cands, q, seqs, k, dt, int, int)

    def operators(self):
        """Trainer.get_close (its length window), filter, merge, merge_all / merge_some and update_centres on sparse sets, each
        against the oracle centre by centre: lists of 0, 1 and many members, and members that are all identical (distances tie and the
        first minimum must win); a fast and a `--feat slow` model"""
        k, dt = 9, 16
        fam, _ = synth.families(4606, 24, 1000, family=6, length_jitter=300)
        seqs = list(fam) + [fam[3]] * 4 + [b"ACGT", b"A" * (k + 5)]
        n = len(seqs)
        hs = api.HistogramSet(self.ctx, k, dt, n, sparse_entries=sum(len(s) for s in seqs) + 4096)
        hs.build(seqs)
        same = [24, 25, 26, 27]                              # four slots holding one sequence (and slot 3 too)
        for wts, cutoff in (("weights_k9_u32.txt", 0.9), ("weights_jitter_slow_k9.txt", 0.8)):
            text = weights_text(wts)
            feat = api.Feature.from_text(self.ctx, text, 0)
            trn = api.Trainer(self.ctx, feat, cutoff)
            queries = (0, 3, 13, 27, 28)
            centres = np.array([0, 3, 7, 13, 20, 24, 25, 29], dtype=np.uint32)
            cslots = np.arange(len(centres), dtype=np.uint32)[::-1].copy()      # centre j sits in slot cslots[j] of `cen`
            lists = [np.arange(n, dtype=np.uint32), np.array([], dtype=np.uint32), np.array([5], dtype=np.uint32), np.array(same, dtype=np.uint32),
                     np.array([3] + same, dtype=np.uint32), np.array([1, 2, 4, 6, 8, 10, 12, 14, 28, 29], dtype=np.uint32),
                     np.array([29, 28], dtype=np.uint32), np.array(same[::-1] + [11], dtype=np.uint32)]

            def oracle_values():
                pred = oracle_py.predictor(text)
                oh = [oracle_py.hist(s, k, dt) for s in seqs]
                try:
                    out = {"get_close": [], "filter": [], "merge": {}, "update": []}
                    for q in queries:
                        w = [c for c in range(n) if c != q]
                        out["get_close"].append(oracle_py.get_close(pred, cutoff, oh[q], [oh[c] for c in w]))
                        out["filter"].append(oracle_py.filter_(pred, cutoff, oh[q], [oh[c] for c in w]))
                    cen_oh = [oh[int(centres[j])] for j in range(len(centres))]
                    for delta in (0, 1, 3, 7):
                        out["merge"][delta] = [oracle_py.merge(pred, cutoff, cen_oh, i, i + 1, min(len(centres) - 1, i + delta)) for i in range(len(centres))]
                    for j, lst in enumerate(lists):
                        keep = oracle_py.filter_(pred, cutoff, cen_oh[j], [oh[int(s)] for s in lst]) if len(lst) else np.zeros(0, dtype=np.uint8)
                        idx = np.flatnonzero(keep)
                        near = int(idx[oracle_py.mean_nearest([oh[int(lst[i])] for i in idx])[2]]) if idx.size else -1
                        out["update"].append((near, int(idx.size)))
                    out["mean"] = [oracle_py.mean_nearest([oh[int(s)] for s in lists[j]]) for j in MEAN_LISTS]
                    return out
                finally:
                    for h in oh:
                        oracle_py.lib().orc_hist_free(h)
            exp = self.oracle.cached("operators_" + wts[:-4], oracle_values)
            for t, q in enumerate(queries):
                w = np.array([c for c in range(n) if c != q], dtype=np.uint32)
                flags, bp, bs, im = trn.get_close(hs, w, hs, q)
                of, obp, obs, oim = exp["get_close"][t]
                assert np.array_equal(flags, of) and (bp, im) == (obp, oim), ("get_close", wts, q)
                assert abs(bs - obs) <= 1e-9 * abs(obs), ("get_close", wts, q, bs, obs)
                assert np.array_equal(trn.filter(hs, q, hs, w), exp["filter"][t]), ("filter", wts, q)
            cen = api.HistogramSet(self.ctx, k, dt, len(centres), sparse_entries=sum(len(seqs[int(c)]) for c in centres) + 4096)
            for j, c in enumerate(centres):
                cen.clone_from(int(cslots[j]), hs, int(c))
            for delta in (0, 1, 3, 7):
                best = trn.merge_all(cen, cslots, delta)
                assert list(best) == exp["merge"][delta], ("merge_all", wts, delta, list(best))
                for i in range(len(centres)):
                    assert trn.merge(cen, cslots, i, i + 1, min(len(centres) - 1, i + delta)) == exp["merge"][delta][i], ("merge", wts, delta, i)
                which = np.array([5, 0, 3, 7], dtype=np.uint64)
                assert list(trn.merge_some(cen, cslots, delta, which)) == [exp["merge"][delta][int(i)] for i in which], ("merge_some", wts, delta)
            self.routes["operators_update_grouped"] = mean_grouped(4 ** k, 4 ** k // batch_sweep_chunks(4 ** k, len(centres)))
            self.routes["operators_mean_grouped"] = mean_grouped(4 ** k, 4 ** k // min(1024, 4 ** k // 256))
            nearest, kept = trn.update_centres(cen, cslots, hs, lists)
            for j in range(len(centres)):
                assert (int(nearest[j]), int(kept[j])) == exp["update"][j], ("update_centres", wts, j, nearest[j], kept[j], exp["update"][j])
            for t, j in enumerate(MEAN_LISTS):          # get_mean / closest alone: the distances to the rounded mean, the first nearest member
                pos, d, _ = trn.closest(hs, lists[j])                # (a sparse set does not hand out its dense mean)
                _, od, opos = exp["mean"][t]
                assert pos == opos and np.allclose(d, od, rtol=1e-12, atol=0), ("mean_nearest", wts, j, pos, opos)
                self.dump["mean_operators_%s_%d" % (wts[:-4], j)] = d
            self.qxm(hs, np.array([0, 3, 27, 28, 13, 29], dtype=np.uint32), np.array([c for c in range(n)] + [3, 3, 0], dtype=np.uint32), wts, (seqs, k, dt))

    def qxm(self, hs, qs, cands, wts, oracle_seqs, key=None):
        """score_multi over a sparse set == one 1 x M pass per query, bit for bit (the queued record array of sparse_multi, or the passes
        query by query); the raw statistics of sampled pairs held to the oracle"""
        feat = api.Feature.from_text(self.ctx, weights_text(wts), 0)
        slow = "slow" in wts
        mask = ALL_MASK if slow else INT_MASK
        multi = api.score_multi(self.ctx, feat, hs, cands, hs, qs, feat_mask=mask)
        kern = self.ctx.last_kernel_info()[0]
        if not slow:
            queued = not any(s in ENV for s in ("MSC_SPARSE_NO_MULTI", "MSC_SPARSE_NO_MP", "MSC_SPARSE_LDS"))
            if queued:
                c_max = max(hs.entries(s) for s in range(hs.capacity))
                fit = sum("MSC_SPARSE_NO_WL" not in ENV and hs.entries(int(q)) + 4 * c_max + 10 <= 8192 for q in qs)
                assert kern == ("k_pair_sparse_wl" if fit == len(qs) else "k_pair_sparse_mp+wl" if fit else "k_pair_sparse_mp"), (kern, wts, fit)
        for i, q in enumerate(qs):
            raw = api.pair_features_raw(self.ctx, hs, cands, hs, int(q), mask)
            single = feat.compute(hs, cands, hs, int(q))
            assert np.array_equal(multi["raw"][i], raw, equal_nan=True), ("qxm raw", wts, i)
            assert np.array_equal(multi["sum"][i], single["sum"], equal_nan=True) and np.array_equal(multi["csum"][i], single["csum"], equal_nan=True), ("qxm sum", wts, i)
            assert np.array_equal(multi["close"][i], (np.round(single["csum"]) > 0).astype(np.uint8)), ("qxm close", wts, i)
        if oracle_seqs:
            seqs, k, dt = oracle_seqs
            sample = [(int(cands[j]), int(qs[i])) for i in range(len(qs)) for j in range(i, len(cands), 7)]
            pairs = [(c, q, api.ORDER_CAND_FIRST) for c, q in sample]
            key = key or "qxm_" + wts[:-4]
            exp = self.oracle.raw_table(key, seqs, k, dt, pairs)
            at = [(i, j) for i in range(len(qs)) for j in range(i, len(cands), 7)]
            cols = [i for i, (_, b) in enumerate(FEATS) if mask >> b & 1]
            full = np.zeros((len(pairs), len(FEATS)))
            full[:, cols] = np.array([multi["raw"][i][j] for i, j in at])
            hold(key, full, exp, pairs, cols)

    def means(self):
        """The sparse mean where the mean switches choose its sweep: get_mean / closest at k = 10 (chunks of 1 024 bins: the grouped sweep
        by default, the full one under MSC_SPARSE_MEAN_GROUPS_MIN_K=16 or MSC_SPARSE_MEAN_NO_GROUPS), and update_centres of 300 centres at
        k = 8 (the batched sweep in chunks of 512 bins: grouped only under MSC_SPARSE_MEAN_GROUPS_MIN_K <= 8). Lists of 0, 1 and a few
        members, identical members among them; nearest member and kept count per centre, and the distances, against the oracle. The
        distances of every closest call go to the dump (mean_*): the grouped and the full sweep must give the same list."""
        wts, cutoff = "weights_k9_u32.txt", 0.9
        text = weights_text(wts)
        trn = api.Trainer(self.ctx, api.Feature.from_text(self.ctx, text, 0), cutoff)
        fam, _ = synth.families(4607, 30, 1000, family=6, length_jitter=200)
        seqs = list(fam) + [fam[4]] * 3
        n = len(seqs)
        # k = 10: closest alone
        k, dt = 10, 16
        hs = api.HistogramSet(self.ctx, k, dt, n, sparse_entries=sum(len(s) for s in seqs) + 4096)
        hs.build(seqs)
        lists = [np.arange(n, dtype=np.uint32), np.array([7], dtype=np.uint32), np.array([30, 4, 31, 32], dtype=np.uint32),
                 np.array([1, 2, 3, 5, 8, 13, 21], dtype=np.uint32)]

        def closest_oracle():
            oh = [oracle_py.hist(s, k, dt) for s in seqs]
            try:
                return [oracle_py.mean_nearest([oh[int(s)] for s in lst])[1:] for lst in lists]
            finally:
                for h in oh:
                    oracle_py.lib().orc_hist_free(h)
        exp = self.oracle.cached("means_k10", closest_oracle)
        self.routes["means_k10_grouped"] = mean_grouped(4 ** k, 4 ** k // min(1024, 4 ** k // 256))
        for t, (lst, (od, opos)) in enumerate(zip(lists, exp)):
            pos, d, _ = trn.closest(hs, lst)
            assert pos == opos and np.allclose(d, od, rtol=1e-12, atol=0), ("closest k10", list(lst), pos, opos)
            self.dump["mean_k10_%d" % t] = d
        # the first n slots without a slot list (the one route with a null list; always the full sweep) == the same slots listed
        pos, d, _ = trn.closest(hs, None, m=n)
        pos_l, d_l, _ = trn.closest(hs, np.arange(n, dtype=np.uint32))
        assert pos == pos_l and np.array_equal(d, d_l), ("closest without a list", pos, pos_l)
        self.dump["mean_k10_no_list"], self.dump["mean_k10_listed"] = d, d_l
        # k = 8: the batched update of 300 centres
        k, dt = 8, 16
        hs = api.HistogramSet(self.ctx, k, dt, n, sparse_entries=sum(len(s) for s in seqs) + 4096)
        hs.build(seqs)
        nc = 300
        cen = api.HistogramSet(self.ctx, k, dt, nc, sparse_entries=nc * 1300 + 4096)
        cslots = np.arange(nc, dtype=np.uint32)[::-1].copy()
        owner = [(7 * j) % n for j in range(nc)]
        for j in range(nc):
            cen.clone_from(int(cslots[j]), hs, owner[j])
        lists = [np.array([], dtype=np.uint32) if j % 9 == 0 else np.array([owner[j]], dtype=np.uint32) if j % 9 == 1 else
                 np.array([30, 31, 32, 4], dtype=np.uint32) if j % 9 == 2 else np.array([(owner[j] + t) % n for t in (0, 1, 2)], dtype=np.uint32)
                 for j in range(nc)]

        def update_oracle():
            pred = oracle_py.predictor(text)
            oh = [oracle_py.hist(s, k, dt) for s in seqs]
            try:
                out = []
                for j, lst in enumerate(lists):
                    keep = oracle_py.filter_(pred, cutoff, oh[owner[j]], [oh[int(s)] for s in lst]) if len(lst) else np.zeros(0, dtype=np.uint8)
                    idx = np.flatnonzero(keep)
                    out.append((int(idx[oracle_py.mean_nearest([oh[int(lst[i])] for i in idx])[2]]) if idx.size else -1, int(idx.size)))
                return out
            finally:
                for h in oh:
                    oracle_py.lib().orc_hist_free(h)
        exp = self.oracle.cached("means_k8_update", update_oracle)
        self.routes["means_k8_update_grouped"] = mean_grouped(4 ** k, 4 ** k // batch_sweep_chunks(4 ** k, nc))
        nearest, kept = trn.update_centres(cen, cslots, hs, lists)
        for j in range(nc):
            assert (int(nearest[j]), int(kept[j])) == exp[j], ("update_centres k8", j, nearest[j], kept[j], exp[j])
        self.means_u8(seqs)

    def means_u8(self, plain):
        """k = 8, u8 (64 KiB: the smallest sparse u8 set), members with a bin saturated at 255 -- poly-A in all of them, poly-G in every
        third: a mean bin of 255 is where a rounding narrower than the bin type's would show. closest, and update_centres of three centres."""
        k, dt = 8, 8
        text, cutoff = weights_text("weights_k8_u16.txt"), 0.9          # (a model that keeps members of the centre's family at k = 8)
        trn = api.Trainer(self.ctx, api.Feature.from_text(self.ctx, text, 0), cutoff)
        seqs = means_u8_seqs(plain, k)
        n = len(seqs)
        hs = api.HistogramSet(self.ctx, k, dt, n, sparse_entries=sum(len(s) for s in seqs) + 4096)
        hs.build(seqs)
        assert all(int(hs.download(i).max()) == 255 for i in range(n))
        lists, owner, ulists = means_u8_lists(n)
        exp = self.oracle.cached("means_k8_u8", lambda: means_u8_oracle(seqs, k, dt, text, cutoff))
        assert all(c >= 1 for c in exp["bins_255"]) and exp["bins_255"][1] >= 2 and max(kept for _, kept in exp["update"]) >= 3, exp
        for t, (lst, (od, opos)) in enumerate(zip(lists, exp["closest"])):
            pos, d, _ = trn.closest(hs, lst)
            assert pos == opos and np.allclose(d, od, rtol=1e-12, atol=0), ("closest k8 u8", list(lst), pos, opos)
            self.dump["mean_k8_u8_%d" % t] = d
        cen = api.HistogramSet(self.ctx, k, dt, len(owner), sparse_entries=len(owner) * 2500 + 4096)
        cslots = np.arange(len(owner), dtype=np.uint32)[::-1].copy()
        for j, o in enumerate(owner):
            cen.clone_from(int(cslots[j]), hs, o)
        nearest, kept = trn.update_centres(cen, cslots, hs, ulists)
        for j in range(len(owner)):
            assert (int(nearest[j]), int(kept[j])) == exp["update"][j], ("update_centres k8 u8", j, nearest[j], kept[j], exp["update"][j])

    def save(self):
        os.makedirs(self.out_dir, exist_ok=True)
        for name, a in self.dump.items():
            np.save(os.path.join(self.out_dir, name + ".npy"), a)
        with open(os.path.join(self.out_dir, "routes.json"), "w") as f:
            json.dump(self.routes, f, sort_keys=True)


def means_u8_seqs(plain, k):
    """the members of Check.means_u8: every sequence with a run that saturates the u8 bin of poly-A, every third also that of poly-G"""
    return [s[:300] + run_of(b"A", 300, k) + s[300:] + (run_of(b"G", 300, k) if i % 3 == 0 else b"") for i, s in enumerate(plain)]


def means_u8_lists(n):
    """-> (lists for closest: all members, members that all hold both saturated bins, members of which some do; the owner sequence of
    each of three centres; their neighbourhoods: sequence 4 and its copies 30 .. 32 (30 with the poly-G run), the copies, everything)"""
    lists = [np.arange(n, dtype=np.uint32), np.array([0, 3, 6, 9], dtype=np.uint32), np.array([1, 2, 3, 4, 5], dtype=np.uint32)]
    return lists, [4, 31, 0], [np.array([4, 31, 32, 30, 5], dtype=np.uint32), np.array([30, 31, 32], dtype=np.uint32), np.arange(n, dtype=np.uint32)]


def means_u8_oracle(seqs, k, dt, text, cutoff):
    """oracle_py.mean_nearest of every list of means_u8_lists (distances, nearest, how many bins of the rounded mean are 255) and the
    (nearest survivor, survivors) of the three centres"""
    lists, owner, ulists = means_u8_lists(len(seqs))
    pred = oracle_py.predictor(text)
    oh = [oracle_py.hist(s, k, dt) for s in seqs]
    try:
        out = {"closest": [], "bins_255": [], "update": []}
        for lst in lists:
            mean, d, pos = oracle_py.mean_nearest([oh[int(s)] for s in lst])
            out["closest"].append((d, pos))
            out["bins_255"].append(int((np.round(mean) == 255).sum()))
        for o, lst in zip(owner, ulists):
            idx = np.flatnonzero(oracle_py.filter_(pred, cutoff, oh[o], [oh[int(s)] for s in lst]))
            out["update"].append((int(idx[oracle_py.mean_nearest([oh[int(lst[i])] for i in idx])[2]]) if idx.size else -1, int(idx.size)))
        return out
    finally:
        for h in oh:
            oracle_py.lib().orc_hist_free(h)


def batch_sweep_chunks(nbins, nc):
    """chunks of bins the batched sparse mean of nc centres is swept in (msc_api_batch.hip sparse_sweep_chunks)"""
    n_chunks = min(1024, nbins // 256)
    while n_chunks > 16 and n_chunks * nc > 65536:
        n_chunks //= 2
    return n_chunks


def hold(name, got, exp, pairs, cols=None):
    """GPU raw statistics [pairs, 11] against the oracle's [pairs, 13]: integer statistics equal (kulczynski2 to 1e-9 relative, as in
    test_gpu_parity), the other FP64 statistics to 1e-9 relative, the divergences also to an extended-precision evaluation at 1e-10"""
    for c in (range(len(FEATS)) if cols is None else cols):
        feat = FEATS[c][0]
        for t in range(len(pairs)):
            g, e = got[t, c], exp[t, c]
            if np.isnan(e):
                ok = bool(np.isnan(g))          # (pearson of a list with no stored bin: a constant histogram, as in the reference)
            elif feat in EXACT and feat != "kulczynski2":
                ok = g == e
            else:
                ok = abs(g - e) <= 1e-9 * abs(e) + 1e-13
            if ok and feat in DIV:
                ld = exp[t, len(FEATS) + DIV.index(feat)]
                ok = abs(g - ld) <= 1e-10 * abs(ld) + 1e-18
            assert ok, (name, feat, pairs[t], g, e, exp[t, len(FEATS):])


def main():
    out_dir = sys.argv[1]
    cache = sys.argv[2] if len(sys.argv) > 2 else None
    # STARTED before the first GPU call, DONE after the last check: a variant that left STARTED alone ran and failed, and is not run again
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "STARTED"), "w").close()
    chk = Check(out_dir, cache)
    for case in (chk.chunk_ends, lambda: chk.chunk_ends(12, 16, (1, 2), (-1, 1)), chk.degenerate, chk.unequal_and_parts, chk.wl_boundary,
                 chk.count_boundary, chk.operators, chk.means):
        case()
        print("ok", getattr(case, "__name__", "case"), flush=True)
    chk.save()
    open(os.path.join(out_dir, "DONE"), "w").close()
    print("SPARSE_ROUTE_OK", chk.n_calls, "calls")


if __name__ == "__main__":
    main()
