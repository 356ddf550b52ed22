"""Host-side mirror of the reference's interface for the hot path, over the C ABI.

Names follow the reference: Loader::get_point -> HistogramSet.build, Feature::compute ->
Feature.compute / raw, Trainer::get_close / filter / merge / closest -> Trainer.*, Predictor::close /
similarity -> Predictor.*. Everything here is plumbing (ctypes marshalling); the work happens in
libmeshclust2_hip.so on the GPU.
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import FEAT, FEAT_FAST, FEAT_SLOW, MscError, ORDER_CAND_FIRST, ORDER_QUERY_FIRST, PAIRS_ROUTE_FALLBACK, PAIRS_ROUTE_MATRIX  # noqa: F401

NP_T = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context:
    """One HIP device + stream (msc_ctx). Not thread-safe: one per host thread."""

    def __init__(self, device=0):
        self.lib = _capi.load_library()
        h = C.c_void_p()
        rc = self.lib.msc_create(int(device), C.byref(h))
        if rc != 0:
            raise MscError(rc, self.lib.msc_last_error(None).decode())
        self.h = h
        self.device = device
        self._children = []          # weakrefs to sets / models so that close() can release them before the ctx
        self._pinned = []            # page-locked host arrays handed out by pinned_array

    def _adopt(self, obj):
        self._children.append(weakref.ref(obj))

    def check(self, rc):
        if rc != 0:
            raise MscError(rc, self.lib.msc_last_error(self.h).decode())

    def device_name(self):
        buf = C.create_string_buffer(256)
        self.check(self.lib.msc_device_name(self.h, buf, 256))
        return buf.value.decode()

    def synchronize(self):
        self.check(self.lib.msc_synchronize(self.h))

    def last_kernel_ms(self):
        """(pair_tiles ms, whole device pipeline ms) of the last scoring call, from HIP events on the ctx stream."""
        a, b = C.c_float(), C.c_float()
        self.check(self.lib.msc_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_kernel_timing(self, on):
        """the HIP events behind last_kernel_ms: off for step-serial loops (four event records per call)"""
        self.check(self.lib.msc_set_kernel_timing(self.h, 1 if on else 0))

    def set_mirror_pass(self, on):
        """dense sets: 1 x M passes over the sparse mirror (default) or over the bins with the streaming kernel; same results"""
        self.check(self.lib.msc_set_mirror_pass(self.h, 1 if on else 0))

    def set_block_pipe(self, on):
        """msc_score_multi's blocks on three streams (default) or every kernel of a block on one: same results, unstretched kernel timings"""
        self.check(self.lib.msc_set_block_pipe(self.h, 1 if on else 0))

    def set_pairs_div_cells(self, on):
        """search_pairs with a divergence-statistic (--feat slow) model: the matrix-core route with the two sums from cells (on) or the
        fallback through score_multi (default); similarities agree to rounding (1e-9 relative), not bit for bit"""
        self.check(self.lib.msc_set_pairs_div_cells(self.h, 1 if on else 0))

    def set_multi_div_cells(self, on):
        """score_multi with a divergence statistic in the model or the mask: the matrix-core route with the two sums from cells and no merge
        pass per query (on) or the merge passes behind the product (default); every other statistic is bit-equal, the two sums and what
        a model derives from them agree to rounding (1e-9 relative), not bit for bit"""
        self.check(self.lib.msc_set_multi_div_cells(self.h, 1 if on else 0))

    def set_emd_bounds(self, on):
        """score_multi's close flags with an earth_movers_distance model: decided from bounds of the distance, rank lists walked for the
        pairs the bounds leave open only (default), or the distance of every pair formed first (off); the same flags"""
        self.check(self.lib.msc_set_emd_bounds(self.h, 1 if on else 0))

    def last_emd_walk(self):
        """(listed_pairs, dense_blocks, blocks) of the last score_multi call: pairs whose rank lists were walked one by one, close-flag
        blocks whose every pair was walked, and such blocks in all (a block whose candidates run in several chunks counts once per chunk)"""
        v = [C.c_uint64(0) for _ in range(3)]
        self.check(self.lib.msc_last_emd_walk(self.h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2])))
        return tuple(int(x.value) for x in v)

    def set_fold_screen(self, fold):
        """score_multi's close-flag blocks with an earth_movers_distance model: the matrix product over presence bits folded `fold`-to-1
        (8, 16 -- the default -- or 32) with the screen deciding from intervals and exact counts for the pairs it leaves open, or the true
        product (0); the same flags"""
        self.check(self.lib.msc_set_fold_screen(self.h, int(fold)))

    def set_query_groups(self, cap):
        """score_multi's matrix-core blocks: the queries' side of up to `cap` consecutive full blocks in one set of launches (default 32), or
        block by block (0 or 1); identical results"""
        self.check(self.lib.msc_set_query_groups(self.h, int(cap)))

    def set_tail_groups(self, cap):
        """score_multi's folded blocks: what follows the product of up to `cap` consecutive full blocks of one query group in one set of
        launches (default 8), or block by block (0 or 1); identical results and counters"""
        self.check(self.lib.msc_set_tail_groups(self.h, int(cap)))

    def last_tail_groups(self):
        """(groups, grouped_blocks) of the last score_multi call: the tail groups of two blocks and more it ran, and the blocks in them"""
        v = [C.c_uint64(0) for _ in range(2)]
        self.check(self.lib.msc_last_tail_groups(self.h, C.byref(v[0]), C.byref(v[1])))
        return tuple(int(x.value) for x in v)

    def last_fold_screen(self):
        """(fold, folded_blocks, fell_back) of the last score_multi call: the fold used (0: none), the blocks whose product was folded and
        those of them whose list of open pairs overflowed and were scored again with the true product"""
        v = [C.c_uint64(0) for _ in range(3)]
        self.check(self.lib.msc_last_fold_screen(self.h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2])))
        return tuple(int(x.value) for x in v)

    def set_fold_reject(self, on):
        """score_multi's folded blocks: an integer cut per query row, proven once per block, decides the pairs whose folded product output
        lies under it without an evaluation (default), or every pair goes through the screen; the same flags"""
        self.check(self.lib.msc_set_fold_reject(self.h, 1 if on else 0))

    def last_fold_reject(self):
        """(rejected_pairs, rows_without_cut) of the last score_multi call: the pairs of its folded blocks the cut rejected, and the query
        rows of those blocks that got no cut"""
        v = [C.c_uint64(0) for _ in range(2)]
        self.check(self.lib.msc_last_fold_reject(self.h, C.byref(v[0]), C.byref(v[1])))
        return tuple(int(x.value) for x in v)

    def set_sparse_matrix_pass(self, on):
        """score_multi / search_pairs over two sparse sets: the matrix-core route over mirrors built from the lists (on) or one 1 x M pass
        per query (default); identical results"""
        self.check(self.lib.msc_set_sparse_matrix_pass(self.h, 1 if on else 0))

    def device_malloc(self, nbytes):
        """plain device memory of this context's GPU (msc_device_malloc) -> integer device address; release with device_free"""
        p = C.c_void_p()
        self.check(self.lib.msc_device_malloc(self.h, int(nbytes), C.byref(p)))
        return p.value

    def device_free(self, dev_ptr):
        self.check(self.lib.msc_device_free(self.h, C.c_void_p(dev_ptr)))

    def memcpy_to_host(self, dev_src, nbytes):
        """nbytes of device memory at dev_src -> a new uint8 host array (waits for the ctx stream)"""
        out = np.zeros(int(nbytes), dtype=np.uint8)
        self.check(self.lib.msc_memcpy_to_host(self.h, _ptr(out), C.c_void_p(dev_src), int(nbytes)))
        return out

    def memcpy_to_device(self, dev_dst, host):
        """a host array's bytes -> device memory at dev_dst (waits for the ctx stream)"""
        a = np.ascontiguousarray(host)
        self.check(self.lib.msc_memcpy_to_device(self.h, C.c_void_p(dev_dst), _ptr(a), a.nbytes))

    def last_kernel_launches(self):
        return self.lib.msc_last_kernel_launches(self.h)

    def last_kernel_info(self):
        """-> (name of the streaming kernel the last scoring call ran, queries served per HBM read of a candidate tile)"""
        buf = C.create_string_buffer(256)
        n = C.c_int()
        self.check(self.lib.msc_last_kernel_info(self.h, buf, 256, C.byref(n)))
        return buf.value.decode(), n.value

    def close(self):
        if getattr(self, "h", None):
            for ref in self._children:
                obj = ref()
                if obj is not None:
                    obj.close()
            self._children = []
            for p in getattr(self, "_pinned", []):
                self.lib.msc_host_free(self.h, C.c_void_p(p))
            self._pinned = []
            self.lib.msc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def encode(seq):
    """Chromosome::help + ChromosomeOneDigit::encode -> (codes, [(s, e)...], effective length)."""
    lib = _capi.load_library()
    seq = seq if isinstance(seq, bytes) else seq.encode()
    codes = np.zeros(max(len(seq), 1), dtype=np.uint8)
    max_segs = len(seq) // 2 + 2
    segs = np.zeros(2 * max_segs, dtype=np.int64)
    n, eff = C.c_size_t(), C.c_uint64()
    rc = lib.msc_encode(seq, len(seq), codes.ctypes.data_as(C.POINTER(C.c_uint8)), segs.ctypes.data_as(C.POINTER(C.c_int64)),
                        max_segs, C.byref(n), C.byref(eff))
    if rc != 0:
        raise MscError(rc, "invalid nucleotide")
    return codes[:len(seq)].tobytes(), [(int(segs[2 * i]), int(segs[2 * i + 1])) for i in range(n.value)], eff.value


class HistogramSet:
    """Device-resident k-mer histograms (the `points` vector of DivergencePoint<T>*)."""

    def __init__(self, ctx, k, dtype, capacity, sparse_entries=0):
        """sparse_entries > 0 -> sparse layout able to hold that many stored bins in total (msc_hist_set_create_sparse)"""
        self.ctx, self.k, self.dtype, self.capacity = ctx, int(k), int(dtype), int(capacity)
        h = C.c_void_p()
        if sparse_entries:
            ctx.check(ctx.lib.msc_hist_set_create_sparse(ctx.h, self.k, self.dtype, self.capacity, int(sparse_entries), C.byref(h)))
        else:
            ctx.check(ctx.lib.msc_hist_set_create(ctx.h, self.k, self.dtype, self.capacity, C.byref(h)))
        self.h = h
        self.nbins = 4 ** self.k
        ctx._adopt(self)

    def nbytes(self):
        return self.ctx.lib.msc_hist_set_bytes(self.h)

    def entries(self, slot):
        return self.ctx.lib.msc_hist_set_entries(self.h, slot)

    def clear(self):
        """msc_hist_set_clear: a sparse set back to empty, its whole entry arena free (compaction target of a centre store)."""
        self.ctx.check(self.ctx.lib.msc_hist_set_clear(self.ctx.h, self.h))

    def build(self, seqs, first_slot=0, strip=False):
        """Loader<T>::get_point for a batch (clutil/Loader.cpp:112-179)."""
        seqs = [s if isinstance(s, bytes) else s.encode() for s in seqs]
        n = len(seqs)
        arr = (C.c_char_p * max(n, 1))(*seqs)
        lens = (C.c_uint64 * max(n, 1))(*[len(s) for s in seqs])
        self.ctx.check(self.ctx.lib.msc_hist_build(self.ctx.h, self.h, first_slot, n, arr, lens, 1 if strip else 0))

    def build_packed(self, first_slot, n_seqs, packed, n_bases, seg_seq, seg_start, seg_end, eff_len, one_mers):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        seg_seq = np.ascontiguousarray(seg_seq, dtype=np.uint32)
        seg_start = np.ascontiguousarray(seg_start, dtype=np.uint64)
        seg_end = np.ascontiguousarray(seg_end, dtype=np.uint64)
        eff_len = np.ascontiguousarray(eff_len, dtype=np.uint64)
        one_mers = np.ascontiguousarray(one_mers, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.msc_hist_build_packed(self.ctx.h, self.h, first_slot, n_seqs, _ptr(packed), int(n_bases), _ptr(seg_seq),
                                                          _ptr(seg_start), _ptr(seg_end), len(seg_seq), _ptr(eff_len), _ptr(one_mers)))

    def build_packed_dev(self, first_slot, n_seqs, packed_dev_ptr, n_bases, seg_seq, seg_start, seg_end, eff_len, one_mers):
        """build_packed with the 2-bit stream already in this device's memory (packed_dev_ptr: an integer device address, e.g. a torch
        tensor's data_ptr()); the segment table and the per-sequence scalars stay host arrays"""
        seg_seq = np.ascontiguousarray(seg_seq, dtype=np.uint32)
        seg_start = np.ascontiguousarray(seg_start, dtype=np.uint64)
        seg_end = np.ascontiguousarray(seg_end, dtype=np.uint64)
        eff_len = np.ascontiguousarray(eff_len, dtype=np.uint64)
        one_mers = np.ascontiguousarray(one_mers, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.msc_hist_build_packed_dev(self.ctx.h, self.h, first_slot, n_seqs, C.c_void_p(int(packed_dev_ptr)), int(n_bases), _ptr(seg_seq),
                                                              _ptr(seg_start), _ptr(seg_end), len(seg_seq), _ptr(eff_len), _ptr(one_mers)))

    def build_info(self):
        """-> (name of the builder the last build* call on this set ran, max_count, max_sum, max_nnz): msc_hist_set_build_info"""
        buf = C.create_string_buffer(64)
        mc, ms, mn = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx.lib.msc_hist_set_build_info(self.h, buf, 64, C.byref(mc), C.byref(ms), C.byref(mn)))
        return buf.value.decode(), mc.value, ms.value, mn.value

    def download(self, slot):
        out = np.zeros(self.nbins, dtype=NP_T[self.dtype])
        self.ctx.check(self.ctx.lib.msc_hist_download(self.ctx.h, self.h, slot, _ptr(out)))
        return out

    def upload(self, slot, bins, length, one_mers=None):
        bins = np.ascontiguousarray(bins, dtype=NP_T[self.dtype])
        assert bins.size == self.nbins
        om = None if one_mers is None else (C.c_uint64 * 4)(*one_mers)
        self.ctx.check(self.ctx.lib.msc_hist_upload(self.ctx.h, self.h, slot, _ptr(bins), int(length), om))

    def lengths(self, first=0, n=None):
        """effective lengths of n consecutive slots (one call)"""
        n = self.capacity - first if n is None else n
        out = np.zeros(n, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.msc_hist_lengths(self.ctx.h, self.h, first, n, _ptr(out)))
        return out

    def info(self, slot):
        hi = _capi.HistInfo()
        self.ctx.check(self.ctx.lib.msc_hist_info_get(self.ctx.h, self.h, slot, C.byref(hi)))
        return dict(mag=hi.mag, length=hi.length, sum=hi.sum, sum_sq=hi.sum_sq, max_count=hi.max_count,
                    one_mers=list(hi.one_mers), stddev=hi.stddev, overflow=hi.overflow, id=hi.id)

    def set_id(self, slot, id_):
        self.ctx.check(self.ctx.lib.msc_hist_set_id(self.ctx.h, self.h, slot, id_))

    def clone_from(self, dst_slot, src, src_slot):
        """DivergencePoint::clone"""
        self.ctx.check(self.ctx.lib.msc_hist_clone(self.ctx.h, self.h, dst_slot, src.h, src_slot))

    def assign_from(self, dst_slot, src, src_slot):
        """DivergencePoint::set (mag is NOT copied)"""
        self.ctx.check(self.ctx.lib.msc_hist_assign(self.ctx.h, self.h, dst_slot, src.h, src_slot))

    def copy_from(self, dst_slot, src, src_slot):
        """exact copy of a slot (stale magnitude included)"""
        self.ctx.check(self.ctx.lib.msc_hist_copy(self.ctx.h, self.h, dst_slot, src.h, src_slot))

    def clone_batch(self, dst_slots, src, src_slots):
        """DivergencePoint::clone of many slots in one launch per region"""
        d = np.ascontiguousarray(dst_slots, dtype=np.uint32)
        s_ = np.ascontiguousarray(src_slots, dtype=np.uint32)
        assert d.size == s_.size
        self.ctx.check(self.ctx.lib.msc_hist_clone_batch(self.ctx.h, self.h, _ptr(d), src.h, _ptr(s_), d.size))

    def copy_batch(self, dst_slots, src, src_slots):
        """exact copies of many slots in one launch per region"""
        d = np.ascontiguousarray(dst_slots, dtype=np.uint32)
        s_ = np.ascontiguousarray(src_slots, dtype=np.uint32)
        assert d.size == s_.size
        self.ctx.check(self.ctx.lib.msc_hist_copy_batch(self.ctx.h, self.h, _ptr(d), src.h, _ptr(s_), d.size))

    def revcomp_batch(self, dst_slots, src, src_slots):
        """slot dst_slots[i] of this set = the reverse complement of slot src_slots[i] of src (msc_hist_revcomp_batch): bins'[b] = bins[rc(b)],
        the record an exact copy with its 1-mers reversed. Same k, dtype and layout; no in-place form."""
        d = np.ascontiguousarray(dst_slots, dtype=np.uint32)
        s_ = np.ascontiguousarray(src_slots, dtype=np.uint32)
        assert d.size == s_.size
        self.ctx.check(self.ctx.lib.msc_hist_revcomp_batch(self.ctx.h, self.h, _ptr(d), src.h, _ptr(s_), d.size))

    def canonical_batch(self, dst_slots, src, src_slots):
        """slot dst_slots[i] of this set = the strand-neutral form of slot src_slots[i] of src (msc_hist_canonical_batch):
        bins'[b] = clamp(bins[b] + bins[rc(b)] - 1, 0, max(T)), so that a sequence and its reverse complement give the same slot. length and id
        are copied, the 1-mers added up the same way, everything else of the record recomputed. Same k, dtype and layout; with src is self,
        dst_slots[i] == src_slots[i] is the in-place form."""
        d = np.ascontiguousarray(dst_slots, dtype=np.uint32)
        s_ = np.ascontiguousarray(src_slots, dtype=np.uint32)
        assert d.size == s_.size
        self.ctx.check(self.ctx.lib.msc_hist_canonical_batch(self.ctx.h, self.h, _ptr(d), src.h, _ptr(s_), d.size))

    def device_view(self):
        b, s = C.c_void_p(), C.c_void_p()
        sb, ss = C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx.lib.msc_hist_set_device_view(self.h, C.byref(b), C.byref(sb), C.byref(s), C.byref(ss)))
        return b.value, sb.value, s.value, ss.value

    def import_done(self, first_slot, n):
        self.ctx.check(self.ctx.lib.msc_hist_import_done(self.ctx.h, self.h, first_slot, n))

    def packed_bytes(self, slot):
        """size of slot's packed byte range (msc_hist_packed_bytes; a multiple of 16)"""
        return self.ctx.lib.msc_hist_packed_bytes(self.h, int(slot))

    def pack(self, slots, dev_dst, offsets):
        """slots[i] -> device memory dev_dst + offsets[i] (offsets: multiples of 16, ranges disjoint)"""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        of = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert sl.size == of.size
        self.ctx.check(self.ctx.lib.msc_hist_pack(self.ctx.h, self.h, _ptr(sl), sl.size, C.c_void_p(dev_dst), _ptr(of)))

    def unpack(self, slots, dev_src, offsets):
        """device memory dev_src + offsets[i] -> slots[i]: an exact copy of the packed slot (stale magnitude included)"""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        of = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert sl.size == of.size
        self.ctx.check(self.ctx.lib.msc_hist_unpack(self.ctx.h, self.h, _ptr(sl), sl.size, C.c_void_p(dev_src), _ptr(of)))

    def reset(self):
        """msc_hist_set_reset: a sparse set forgets every list (no-op on dense sets)"""
        self.ctx.check(self.ctx.lib.msc_hist_set_reset(self.ctx.h, self.h))

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.msc_hist_set_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _slots(slots, m=None):
    if slots is None:
        return None, int(m)
    a = np.ascontiguousarray(slots, dtype=np.uint32)
    return a, a.size


class Feature:
    """Feature<T> + GLM weights of one weights-file block (msc_model)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        self.k = ctx.lib.msc_model_k(handle)
        self.n_singles = ctx.lib.msc_model_n_singles(handle)
        self.n_combos = ctx.lib.msc_model_n_combos(handle)
        ctx._adopt(self)

    @classmethod
    def from_file(cls, ctx, path, block=0):
        h = C.c_void_p()
        ctx.check(ctx.lib.msc_model_load(ctx.h, path.encode(), block, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_text(cls, ctx, text, block=0):
        h = C.c_void_p()
        ctx.check(ctx.lib.msc_model_parse(ctx.h, text.encode() if isinstance(text, str) else text, block, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def create(cls, ctx, k, combos, weights, singles, bias=0.0):
        """combos: [(kind, flags)], weights: [w0, w1..], singles: [(flag, min, max)]"""
        nc, ns = len(combos), len(singles)
        kinds = (C.c_int * max(nc, 1))(*[c[0] for c in combos])
        flags = (C.c_uint64 * max(nc, 1))(*[c[1] for c in combos])
        w = (C.c_double * (nc + 1))(*weights)
        sf = (C.c_uint64 * max(ns, 1))(*[s[0] for s in singles])
        mn = (C.c_double * max(ns, 1))(*[s[1] for s in singles])
        mx = (C.c_double * max(ns, 1))(*[s[2] for s in singles])
        h = C.c_void_p()
        ctx.check(ctx.lib.msc_model_create(ctx.h, k, nc, kinds, flags, w, ns, sf, mn, mx, bias, C.byref(h)))
        return cls(ctx, h)

    def single_flags(self):
        out = (C.c_uint64 * max(self.n_singles, 1))()
        self.ctx.check(self.ctx.lib.msc_model_single_flags(self.h, out))
        return list(out[:self.n_singles])

    def set_bias(self, b):
        self.ctx.lib.msc_model_set_bias(self.h, b)

    def compute(self, cands, cand_slots, qset, q_slot, order=ORDER_CAND_FIRST, m=None):
        """Feature::compute + operator() + weighted sum for 1 query x m candidates.
        -> dict(singles [m,n_singles], combos [m,n_combos], sum [m], csum [m])"""
        sl, m = _slots(cand_slots, m)
        singles = np.zeros((m, self.n_singles))
        combos = np.zeros((m, self.n_combos))
        s = np.zeros(m)
        cs = np.zeros(m)
        self.ctx.check(self.ctx.lib.msc_score(self.ctx.h, self.h, cands.h, _ptr(sl), m, qset.h, q_slot, order,
                                              _ptr(singles), _ptr(combos), _ptr(s), _ptr(cs)))
        return dict(singles=singles, combos=combos, sum=s, csum=cs)

    def compute_pairs(self, a_set, a_slots, b_set, b_slots, order=ORDER_CAND_FIRST, n=None):
        """Feature::compute + operator() for an explicit list of pairs (a_slots[i] of a_set, b_slots[i] of b_set) in one call
        (msc_score_pair_list) -> (singles [n,n_singles], combos [n,n_combos]), rows in the caller's order"""
        a, b, n = _pair_slots(a_slots, b_slots, n)
        singles = np.zeros((n, self.n_singles))
        combos = np.zeros((n, self.n_combos))
        self.ctx.check(self.ctx.lib.msc_score_pair_list(self.ctx.h, self.h, a_set.h, _ptr(a), b_set.h, _ptr(b), n, order, 0, None,
                                                        _ptr(singles), _ptr(combos), None, None, None))
        return singles, combos

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.msc_model_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pair_features_raw(ctx, cands, cand_slots, qset, q_slot, feat_mask=FEAT_FAST, order=ORDER_CAND_FIRST, m=None):
    """The raw statistics of predict/Feature.cpp for 1 query x m candidates -> [m, popcount(mask)], ascending bit order."""
    sl, m = _slots(cand_slots, m)
    nf = bin(feat_mask).count("1")
    out = np.zeros((m, nf))
    ctx.check(ctx.lib.msc_pair_features_raw(ctx.h, cands.h, _ptr(sl), m, qset.h, q_slot, order, feat_mask, _ptr(out)))
    return out


def fold_bin(bin, nbins, fold):
    """msc_fold_bin: the folded bin of `bin` of a histogram of nbins = 4^k bins, bin mod (nbins / fold) (needs no device)"""
    from . import _capi
    return int(_capi.load_library().msc_fold_bin(int(bin), int(nbins), int(fold)))


def pinned_array(ctx, shape, dtype):
    """a numpy array over page-locked host memory (msc_host_alloc; lives as long as the context): device-to-host copies into it are
    not staged by the runtime. For result arrays that are filled call after call (score_multi's `out`)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = C.c_void_p()
    ctx.check(ctx.lib.msc_host_alloc(ctx.h, n, C.byref(p)))
    ctx._pinned.append(p.value)          # released by Context.close (msc_host_free); the array must not be used after that
    buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def score_multi(ctx, feat, cands, cand_slots, qset, q_slots, order=ORDER_CAND_FIRST, m=None, feat_mask=0, want=("sum", "csum", "close"), out=None):
    """n_q queries x m candidates in one pass over the candidates (all-pairs shape).
    -> dict(sum [n_q,m], csum [n_q,m], close [n_q,m], raw [n_q,m,nf] or None); `want` limits what is copied back;
    out: dict of arrays of those shapes to fill instead of new ones (pinned_array: no allocation, no staged copy per call)"""
    sl, m = _slots(cand_slots, m)
    qs = np.ascontiguousarray(q_slots, dtype=np.uint32)
    nq = qs.size
    nf = bin(feat_mask).count("1")

    def arr(name, shape, dtype):
        a = (out or {}).get(name)
        if a is not None:
            if a.shape != shape or a.dtype != np.dtype(dtype) or not a.flags["C_CONTIGUOUS"]:
                raise ValueError("out[%r] must be a C-contiguous %s array of shape %r" % (name, np.dtype(dtype), shape))
            return a
        return np.zeros(shape, dtype=dtype)
    s = arr("sum", (nq, m), np.float64) if feat is not None and "sum" in want else None
    cs = arr("csum", (nq, m), np.float64) if feat is not None and "csum" in want else None
    close = arr("close", (nq, m), np.uint8) if feat is not None and "close" in want else None
    raw = arr("raw", (nq, m, nf), np.float64) if nf else None
    ctx.check(ctx.lib.msc_score_multi(ctx.h, feat.h if feat is not None else None, cands.h, _ptr(sl), m, qset.h, _ptr(qs), nq, order,
                                      _ptr(s), _ptr(cs), _ptr(close), feat_mask, _ptr(raw)))
    counts = None
    if close is not None and "counts" in want:          # row sums of `close`, from the device where the route keeps them
        counts = np.zeros(nq, dtype=np.uint64)
        if ctx.lib.msc_last_close_counts(ctx.h, _ptr(counts), nq) != 0:
            counts = np.einsum("ij->i", close, dtype=np.uint64)
    return dict(sum=s, csum=cs, close=close, raw=raw, counts=counts)


def _pair_slots(a_slots, b_slots, n=None):
    """the two slot lists of a pair list (None = slots 0 .. n-1) -> (a, b, n)"""
    a = None if a_slots is None else np.ascontiguousarray(a_slots, dtype=np.uint32)
    b = None if b_slots is None else np.ascontiguousarray(b_slots, dtype=np.uint32)
    if a is not None and b is not None and a.size != b.size:
        raise ValueError("a_slots and b_slots are one pair list: equal lengths")
    if a is None and b is None and n is None:
        raise ValueError("n is needed when both slot lists are None")
    n = int(n) if a is None and b is None else (a if a is not None else b).size
    return a, b, n


def score_pair_list(ctx, feat, a_set, a_slots, b_set, b_slots, order=ORDER_CAND_FIRST, feat_mask=0, want=("sum", "csum", "close"), n=None):
    """An explicit list of pairs (a_slots[i] of a_set as the candidate, b_slots[i] of b_set as the query) in one call (msc_score_pair_list):
    row i = what pair_features_raw / Feature.compute give for that one pair, in the caller's order.
    -> dict(sum [n], csum [n], close [n], singles [n,n_singles], combos [n,n_combos], raw [n,nf]); what `want` / feat_mask leave out is None"""
    a, b, n = _pair_slots(a_slots, b_slots, n)
    nf = bin(feat_mask).count("1")
    has = feat is not None
    s = np.zeros(n) if has and "sum" in want else None
    cs = np.zeros(n) if has and "csum" in want else None
    close = np.zeros(n, dtype=np.uint8) if has and "close" in want else None
    singles = np.zeros((n, feat.n_singles)) if has and "singles" in want else None
    combos = np.zeros((n, feat.n_combos)) if has and "combos" in want else None
    raw = np.zeros((n, nf)) if nf else None
    ctx.check(ctx.lib.msc_score_pair_list(ctx.h, feat.h if has else None, a_set.h, _ptr(a), b_set.h, _ptr(b), n, order, feat_mask, _ptr(raw),
                                          _ptr(singles), _ptr(combos), _ptr(s), _ptr(cs), _ptr(close)))
    return dict(sum=s, csum=cs, close=close, singles=singles, combos=combos, raw=raw)


def _align_full(name, ctx, seqs, first, second, params, out):
    """msc_align_pairs / msc_align_pairs_long: the arguments and the outputs of align_pairs"""
    match, mismatch, gap_open, gap_continue = params
    raw = [s if isinstance(s, (bytes, bytearray)) else str(s).encode() for s in seqs]
    a = np.ascontiguousarray(first, dtype=np.uint32)
    b = np.ascontiguousarray(second, dtype=np.uint32)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("first and second are one pair list: one dimension, equal lengths")
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in raw], out=offsets[1:])
    text = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
    if out is None:
        out = tuple(np.zeros(a.size, dtype=np.int32) for _ in range(3))
    score, length, matches = out
    for o in out:
        if o.dtype != np.int32 or o.shape != a.shape or not o.flags.c_contiguous:
            raise ValueError("out: three contiguous int32 arrays of n_pairs")
    lib = ctx.lib if ctx is not None else _capi.load_library()
    rc = getattr(lib, name)(ctx.h if ctx is not None else None, _ptr(text), _ptr(offsets), len(raw), _ptr(a), _ptr(b), a.size, int(match), int(mismatch),
                            int(gap_open), int(gap_continue), _ptr(score), _ptr(length), _ptr(matches))
    if rc != 0:
        raise MscError(rc, lib.msc_last_error(ctx.h).decode() if ctx is not None else name + " needs a Context (a gfx950 device): there is no CPU fallback")
    with np.errstate(divide="ignore", invalid="ignore"):
        identity = matches.astype(np.float64) / length.astype(np.float64)
    return dict(score=score, length=length, matches=matches, identity=identity)


def align_pairs(ctx, seqs, first, second, match=1, mismatch=-1, gap_open=2, gap_continue=1, out=None):
    """The global-alignment identity of listed pairs (msc_align_pairs; the reference's GlobAlignE, what Feature::align computes with the
    default parameters): pair p aligns seqs[first[p]] (the definition's sequence 1 -- ties are not symmetric) with seqs[second[p]]. seqs is a
    list of bytes / str of 1 .. 32 767 bytes each; bytes are compared for equality and nothing else.
    -> dict(score, length, matches: int32 [n_pairs]; identity: float64 [n_pairs] = matches / length), in the caller's order. `out` (a tuple
    of three int32 arrays) receives the integers in place: a refused call leaves them as they were."""
    return _align_full("msc_align_pairs", ctx, seqs, first, second, (match, mismatch, gap_open, gap_continue), out)


def align_pairs_long(ctx, seqs, first, second, match=1, mismatch=-1, gap_open=2, gap_continue=1, out=None):
    """align_pairs for sequences of 1 .. 1 048 575 bytes each (msc_align_pairs_long): the same integers, the same dict; pairs
    within align_pairs's limit run on its kernels, longer ones tile by tile."""
    return _align_full("msc_align_pairs_long", ctx, seqs, first, second, (match, mismatch, gap_open, gap_continue), out)


def align_pairs_trace(ctx, seqs, first, second, match=1, mismatch=-1, gap_open=2, gap_continue=1, out=None):
    """align_pairs's integers and the alignment itself (msc_align_pairs_trace): the path the winners of the recurrence point
    along from the corner, run-length encoded, one uint32 per run = run << 4 | op with BAM's op numbers (7 '=', 8 'X', 1 'I' consumes
    seqs[first[p]], the query, 2 'D' consumes seqs[second[p]], the reference). Sequences of 1 .. 32 767 bytes.
    -> align_pairs's dict and op_offsets: uint64 [n_pairs + 1], ops: uint32 [op_offsets[-1]], the whole list; pair p's runs are
    ops[op_offsets[p]:op_offsets[p + 1]] (cigar_string turns them into text). `out`: a tuple of three int32 arrays of n_pairs and a uint64
    one of n_pairs + 1, left as they were by a refused call."""
    raw = [s if isinstance(s, (bytes, bytearray)) else str(s).encode() for s in seqs]
    a = np.ascontiguousarray(first, dtype=np.uint32)
    b = np.ascontiguousarray(second, dtype=np.uint32)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("first and second are one pair list: one dimension, equal lengths")
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in raw], out=offsets[1:])
    text = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
    if out is None:
        out = tuple(np.zeros(a.size, dtype=np.int32) for _ in range(3)) + (np.zeros(a.size + 1, dtype=np.uint64),)
    if len(out) != 4 or any(o.dtype != (np.int32 if i < 3 else np.uint64) or o.shape != (a.size + (i == 3),) or not o.flags.c_contiguous for i, o in enumerate(out)):
        raise ValueError("out: three contiguous int32 arrays of n_pairs and a uint64 one of n_pairs + 1")
    score, length, matches, op_offsets = out
    name = "msc_align_pairs_trace"
    lib = ctx.lib if ctx is not None else _capi.load_library()
    rc = lib.msc_align_pairs_trace(ctx.h if ctx is not None else None, _ptr(text), _ptr(offsets), len(raw), _ptr(a), _ptr(b), a.size, int(match), int(mismatch), int(gap_open),
                                   int(gap_continue), _ptr(score), _ptr(length), _ptr(matches), _ptr(op_offsets))
    if rc != 0:
        raise MscError(rc, lib.msc_last_error(ctx.h).decode() if ctx is not None else name + " needs a Context (a gfx950 device): there is no CPU fallback")
    ops = align_trace_fetch(ctx, 0, int(op_offsets[-1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        identity = matches.astype(np.float64) / length.astype(np.float64)
    return dict(score=score, length=length, matches=matches, identity=identity, op_offsets=op_offsets, ops=ops)


def align_trace_fetch(ctx, first_word, n_words):
    """words first_word .. first_word + n_words of the op list the last align_pairs_trace on ctx left on the device (msc_align_pairs_trace_fetch)
    -> uint32 [n_words]; a range past the list's end is refused"""
    ops = np.zeros(int(n_words), dtype=np.uint32)
    ctx.check(ctx.lib.msc_align_pairs_trace_fetch(ctx.h, int(first_word), int(n_words), _ptr(ops)))
    return ops


def cigar_string(ops):
    """the runs of one pair (uint32, run << 4 | op) as text, such as "120=1X3I": BAM's letters for the op numbers"""
    return "".join("%d%s" % (int(w) >> 4, "MIDNSHP=X"[int(w) & 15]) for w in np.asarray(ops, dtype=np.uint32))


def _align_over_a_band(name, ctx, seqs, first, second, band, params, out, last):
    """msc_align_pairs_banded / msc_align_pairs_auto: align_pairs's arguments, a band between the parameters and the outputs and a fourth
    output (`last`: uint8 flags or uint32 bands)"""
    raw = [s if isinstance(s, (bytes, bytearray)) else str(s).encode() for s in seqs]
    a = np.ascontiguousarray(first, dtype=np.uint32)
    b = np.ascontiguousarray(second, dtype=np.uint32)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("first and second are one pair list: one dimension, equal lengths")
    if not 0 <= int(band) <= 0xffffffff:
        raise ValueError("a band is a uint32")
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in raw], out=offsets[1:])
    text = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
    if out is None:
        out = tuple(np.zeros(a.size, dtype=np.int32) for _ in range(3)) + (np.zeros(a.size, dtype=last),)
    if len(out) != 4 or any(o.dtype != (np.int32 if i < 3 else last) or o.shape != a.shape or not o.flags.c_contiguous for i, o in enumerate(out)):
        raise ValueError("out: three contiguous int32 arrays of n_pairs and one of %s" % np.dtype(last).name)
    lib = ctx.lib if ctx is not None else _capi.load_library()
    rc = getattr(lib, name)(ctx.h if ctx is not None else None, _ptr(text), _ptr(offsets), len(raw), _ptr(a), _ptr(b), a.size, *[int(v) for v in params], int(band),
                            *[_ptr(o) for o in out])
    if rc != 0:
        raise MscError(rc, lib.msc_last_error(ctx.h).decode() if ctx is not None else name + " needs a Context (a gfx950 device): there is no CPU fallback")
    score, length, matches = out[:3]
    with np.errstate(divide="ignore", invalid="ignore"):
        identity = matches.astype(np.float64) / length.astype(np.float64)
    return dict(score=score, length=length, matches=matches, identity=identity), out[3]


def align_pairs_banded(ctx, seqs, first, second, band, match=1, mismatch=-1, gap_open=2, gap_continue=1, out=None):
    """align_pairs over the diagonals within `band` of the corner-to-corner ones only (msc_align_pairs_banded).
    -> align_pairs's dict and certified: uint8 [n_pairs], 1 where the pair's integers are proven to be align_pairs's. `out`: a tuple of three
    int32 arrays and a uint8 one, left as they were by a refused call."""
    r, flags = _align_over_a_band("msc_align_pairs_banded", ctx, seqs, first, second, band, (match, mismatch, gap_open, gap_continue), out, np.uint8)
    r["certified"] = flags
    return r


def align_pairs_auto(ctx, seqs, first, second, match=1, mismatch=-1, gap_open=2, gap_continue=1, first_band=0, out=None):
    """align_pairs's integers, computed over a band that is doubled per pair until the pair is certified (msc_align_pairs_auto; first_band 0:
    the library's default). -> align_pairs's dict and band_used: uint32 [n_pairs], the band that certified the pair, 0xffffffff where the
    full grid was filled. `out`: a tuple of three int32 arrays and a uint32 one, left as they were by a refused call."""
    r, bands = _align_over_a_band("msc_align_pairs_auto", ctx, seqs, first, second, first_band, (match, mismatch, gap_open, gap_continue), out, np.uint32)
    r["band_used"] = bands
    return r


def align_pairs_long_banded(ctx, seqs, first, second, band, match=1, mismatch=-1, gap_open=2, gap_continue=1, out=None):
    """align_pairs_banded for sequences of 1 .. 1 048 575 bytes each (msc_align_pairs_long_banded): the same dict."""
    r, flags = _align_over_a_band("msc_align_pairs_long_banded", ctx, seqs, first, second, band, (match, mismatch, gap_open, gap_continue), out, np.uint8)
    r["certified"] = flags
    return r


def align_pairs_long_auto(ctx, seqs, first, second, match=1, mismatch=-1, gap_open=2, gap_continue=1, first_band=0, out=None):
    """align_pairs_auto for sequences of 1 .. 1 048 575 bytes each (msc_align_pairs_long_auto): the same dict; a long pair's
    band is doubled up to its shorter length."""
    r, bands = _align_over_a_band("msc_align_pairs_long_auto", ctx, seqs, first, second, first_band, (match, mismatch, gap_open, gap_continue), out, np.uint32)
    r["band_used"] = bands
    return r


class Trainer:
    """The pair-scoring operators of cluster/Trainer.{h,cpp} (scoring half only; training is host work out of scope)."""

    def __init__(self, ctx, feat, cutoff):
        self.ctx, self.feat, self.cutoff = ctx, feat, float(cutoff)

    def get_close(self, points, cand_slots, qset, q_slot, m=None):
        """-> (close_flags[m], best_pos, best_sim, is_min)"""
        sl, m = _slots(cand_slots, m)
        flags = np.zeros(max(m, 1), dtype=np.uint8)
        bp, bs, im = C.c_int64(), C.c_double(), C.c_int()
        self.ctx.check(self.ctx.lib.msc_get_close(self.ctx.h, self.feat.h, self.cutoff, points.h, _ptr(sl), m, qset.h, q_slot,
                                                  _ptr(flags), C.byref(bp), C.byref(bs), C.byref(im)))
        return flags[:m], bp.value, bs.value, bool(im.value)

    def filter(self, centre_set, centre_slot, points, pt_slots, m=None):
        """-> keep[m] (1 = survives Trainer::filter)"""
        sl, m = _slots(pt_slots, m)
        keep = np.zeros(max(m, 1), dtype=np.uint8)
        n = C.c_uint64()
        self.ctx.check(self.ctx.lib.msc_filter(self.ctx.h, self.feat.h, self.cutoff, centre_set.h, centre_slot, points.h, _ptr(sl), m,
                                               _ptr(keep), C.byref(n)))
        return keep[:m]

    def merge(self, centres, centre_slots, current, begin, last, n=None):
        sl, n = _slots(centre_slots, n)
        out = C.c_int64()
        self.ctx.check(self.ctx.lib.msc_merge(self.ctx.h, self.feat.h, self.cutoff, centres.h, _ptr(sl), n, current, begin, last, C.byref(out)))
        return out.value

    def merge_all(self, centres, centre_slots, delta):
        """every Trainer::merge call of ClusterFactory's merge loop at once -> best[n] (what merge(i, i+1, min(n-1, i+delta)) returns)"""
        sl = np.ascontiguousarray(centre_slots, dtype=np.uint32)
        best = np.zeros(sl.size, dtype=np.int64)
        self.ctx.check(self.ctx.lib.msc_merge_all(self.ctx.h, self.feat.h, self.cutoff, centres.h, _ptr(sl), sl.size, int(delta), _ptr(best)))
        return best

    def merge_some(self, centres, centre_slots, delta, which):
        """... for the centres which[w] only -> best[len(which)]"""
        sl = np.ascontiguousarray(centre_slots, dtype=np.uint32)
        wh = np.ascontiguousarray(which, dtype=np.uint64)
        best = np.zeros(wh.size, dtype=np.int64)
        self.ctx.check(self.ctx.lib.msc_merge_some(self.ctx.h, self.feat.h, self.cutoff, centres.h, _ptr(sl), sl.size, int(delta), _ptr(wh), wh.size, _ptr(best)))
        return best

    def update_centres(self, centres, centre_slots, points, lists):
        """mean_shift_update for many centres: lists[c] = point slots of centre c's neighbourhood.
        -> (nearest_pos[n] (position inside lists[c], -1 if nothing survives the filter), n_kept[n])"""
        cs = np.ascontiguousarray(centre_slots, dtype=np.uint32)
        flat, offsets = _flat_lists(lists)
        nearest = np.zeros(cs.size, dtype=np.int64)
        kept = np.zeros(cs.size, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.msc_update_centres(self.ctx.h, self.feat.h, self.cutoff, centres.h, _ptr(cs), cs.size, points.h, _ptr(flat), _ptr(offsets),
                                                       _ptr(nearest), _ptr(kept)))
        return nearest, kept

    def filter_batch(self, centres, centre_slots, points, lists):
        """Trainer::filter of centre c against lists[c] for every c in one pass (msc_filter_batch) -> keep, one uint8 array per list"""
        cs = np.ascontiguousarray(centre_slots, dtype=np.uint32)
        assert cs.size == len(lists)
        flat, offsets = _flat_lists(lists)
        keep = np.zeros(max(flat.size, 1), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.msc_filter_batch(self.ctx.h, self.feat.h, self.cutoff, centres.h, _ptr(cs), cs.size, points.h, _ptr(flat), _ptr(offsets),
                                                     _ptr(keep)))
        return [keep[offsets[c]:offsets[c + 1]] for c in range(cs.size)]

    def closest(self, points, member_slots, m=None, want_mean=False):
        """get_mean / closest: -> (nearest_pos, dists[m], mean or None)"""
        sl, m = _slots(member_slots, m)
        d = np.zeros(m)
        mean = np.zeros(points.nbins) if want_mean else None
        pos = C.c_int64()
        self.ctx.check(self.ctx.lib.msc_mean_nearest(self.ctx.h, points.h, _ptr(sl), m, C.byref(pos), _ptr(d), _ptr(mean)))
        return pos.value, d, mean


class Window:
    """The length-sorted store of the accumulate loop kept on the device (msc_window): position i = slot slots[i] of `points`,
    alive until a get_close marks it or kill() removes it."""

    def __init__(self, ctx, points, slots):
        self.ctx, self.points = ctx, points
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        h = C.c_void_p()
        ctx.check(ctx.lib.msc_window_create(ctx.h, points.h, _ptr(sl), sl.size, C.byref(h)))
        self.h, self.n = h, sl.size
        ctx._adopt(self)

    def alive(self, first=0, end=None):
        return self.ctx.lib.msc_window_alive(self.h, first, self.n if end is None else end)

    def kill(self, positions):
        p = np.ascontiguousarray(positions, dtype=np.uint32)
        self.ctx.check(self.ctx.lib.msc_window_kill(self.ctx.h, self.h, _ptr(p), p.size))

    def last_compaction(self):
        """(blocks, threads) of the compaction launch of the last get_close; (0, 0): it returned before launching"""
        b, t = C.c_uint32(), C.c_uint32()
        self.ctx.lib.msc_window_last_compaction(self.h, C.byref(b), C.byref(t))
        return b.value, t.value

    def last_close_blocks(self):
        """workgroups of the last get_close's close pass as a kernel of its own; 0: it rode in the fused epilogue + reduce kernel"""
        return self.ctx.lib.msc_window_last_close_blocks(self.h)

    def get_close(self, trainer, first, end, qset, q_slot):
        """Trainer::get_close over the alive positions of [first, end) -> (close positions (ascending; they die), best position, best_sim, is_min)"""
        lst = C.POINTER(C.c_uint32)()
        n, bp, bs, im = C.c_uint64(), C.c_int64(), C.c_double(), C.c_int()
        self.ctx.check(self.ctx.lib.msc_get_close_window(self.ctx.h, trainer.feat.h, trainer.cutoff, self.h, first, end, qset.h, q_slot, C.byref(lst), C.byref(n),
                                                         C.byref(bp), C.byref(bs), C.byref(im)))
        close = np.ctypeslib.as_array(lst, shape=(n.value,)).astype(np.int64) if n.value else np.zeros(0, dtype=np.int64)
        return close, bp.value, bs.value, bool(im.value)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.msc_window_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_class(ctx, points, first_slots, second_slots, vals, n_train, feat_flags, min_feat, max_feat, ident):
    """Predictor::train's selection + GLM on labelled pairs -> (weights file text, training accuracy, testing accuracy)"""
    fs = np.ascontiguousarray(first_slots, dtype=np.uint32)
    ss = np.ascontiguousarray(second_slots, dtype=np.uint32)
    va = np.ascontiguousarray(vals, dtype=np.float64)
    buf = C.create_string_buffer(1 << 16)
    a, b = C.c_double(), C.c_double()
    ctx.check(ctx.lib.msc_train_class(ctx.h, points.h, _ptr(fs), _ptr(ss), _ptr(va), n_train, fs.size - n_train, feat_flags, min_feat, max_feat, ident,
                                      buf, len(buf), C.byref(a), C.byref(b)))
    return buf.value.decode(), a.value, b.value


def train_regr(ctx, points, first_slots, second_slots, vals, n_train, feat_flags, max_feat, ident):
    """Predictor::train_regr's greedy selection + GLM on labelled pairs -> (weights file text (mode 2), training error, testing error)"""
    fs = np.ascontiguousarray(first_slots, dtype=np.uint32)
    ss = np.ascontiguousarray(second_slots, dtype=np.uint32)
    va = np.ascontiguousarray(vals, dtype=np.float64)
    buf = C.create_string_buffer(1 << 16)
    a, b = C.c_double(), C.c_double()
    ctx.check(ctx.lib.msc_train_regr(ctx.h, points.h, _ptr(fs), _ptr(ss), _ptr(va), n_train, fs.size - n_train, feat_flags, max_feat, ident, buf, len(buf),
                                     C.byref(a), C.byref(b)))
    return buf.value.decode(), a.value, b.value


def mean_nearest(ctx, points, member_slots, m=None, want_mean=False):
    return Trainer(ctx, None, 1.0).closest(points, member_slots, m, want_mean)


def _flat_lists(lists):
    """lists of slots -> (flat uint32 slots, uint64 offsets[len(lists) + 1])"""
    offsets = np.zeros(len(lists) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint32) for x in lists]) if len(lists) else np.zeros(0), dtype=np.uint32)
    return flat, offsets


def colsum_partial(ctx, points, lists):
    """msc_colsum_partial: this rank's integer column sums of lists[c] (slots of `points`) -> a host copy of the payload (uint8).
    Dense sets: uint64 [n][padded bins] then uint64 [n] member counts, to be summed across ranks; sparse sets: a table and packed
    sparse slots, to be gathered across ranks. (The library's buffer is only valid until its next call: it is copied out here.)"""
    flat, offsets = _flat_lists(lists)
    p, nb = C.c_void_p(), C.c_uint64()
    ctx.check(ctx.lib.msc_colsum_partial(ctx.h, points.h, _ptr(flat), _ptr(offsets), len(lists), C.byref(p), C.byref(nb)))
    return ctx.memcpy_to_host(p.value, nb.value)


def colsum_nearest(ctx, points, lists, dev_global, bytes_per_rank, world):
    """msc_colsum_nearest over the reduced (dense) or gathered (sparse, bytes_per_rank apart) payloads at device address dev_global
    -> (pos[n] inside this rank's lists[c] or -1, dist[n], m_total[n] members of list c over all ranks)"""
    flat, offsets = _flat_lists(lists)
    n = len(lists)
    pos = np.zeros(n, dtype=np.int64)
    dist = np.zeros(n)
    m_total = np.zeros(n, dtype=np.uint64)
    ctx.check(ctx.lib.msc_colsum_nearest(ctx.h, points.h, _ptr(flat), _ptr(offsets), n, C.c_void_p(dev_global), int(bytes_per_rank), int(world),
                                         _ptr(pos), _ptr(dist), _ptr(m_total)))
    return pos, dist, m_total


class Predictor:
    """Predictor::close / similarity (predict/Predictor.cpp:255-333) for one query against a database. Like fastcar's work()
    (fastcar/FC_Runner.cpp:432,446-458) it follows the weights file's mode: no classification block -> every entry is close,
    no regression block -> every similarity is 1."""

    def __init__(self, ctx, cls_feat, reg_feat=None):
        self.ctx, self.cls, self.reg = ctx, cls_feat, reg_feat

    @classmethod
    def from_text(cls, ctx, text):
        mode = 0
        for ln in text.splitlines():
            if ln.startswith("mode:"):
                mode = int(ln.split()[1])
                break
        c = Feature.from_text(ctx, text, 0) if mode & 1 else None
        r = Feature.from_text(ctx, text, 1) if mode & 2 else None
        return cls(ctx, c, r)

    @classmethod
    def from_file(cls, ctx, path):
        return cls.from_text(ctx, open(path).read())

    def search(self, db, db_slots, qset, q_slot, m=None):
        sl, m = _slots(db_slots, m)
        close = np.zeros(max(m, 1), dtype=np.uint8)
        sim = np.zeros(max(m, 1))
        self.ctx.check(self.ctx.lib.msc_search(self.ctx.h, self.cls.h if self.cls else None, self.reg.h if self.reg else None, db.h, _ptr(sl), m,
                                               qset.h, q_slot, _ptr(close), _ptr(sim)))
        return close[:m], sim[:m]

    def score_pairs(self, db, a_slots, qset, b_slots, n=None):
        """search() for an explicit list of pairs (a_slots[i] of db against query b_slots[i] of qset) -> (close [n], sim [n]) with msc_search's
        rules per pair: no classification block -> close, no regression block -> similarity 1, else clamp(p_predict, 0, 1). One
        msc_score_pair_list call per model block."""
        a, b, n = _pair_slots(a_slots, b_slots, n)
        lib, h = self.ctx.lib, self.ctx.h
        close = np.ones(n, dtype=np.uint8)
        sim = np.ones(n)
        if self.cls is not None:
            self.ctx.check(lib.msc_score_pair_list(h, self.cls.h, db.h, _ptr(a), qset.h, _ptr(b), n, ORDER_CAND_FIRST, 0, None, None, None, None, None, _ptr(close)))
        if self.reg is not None:
            self.ctx.check(lib.msc_score_pair_list(h, self.reg.h, db.h, _ptr(a), qset.h, _ptr(b), n, ORDER_CAND_FIRST, 0, None, None, None, _ptr(sim), None, None))
            np.clip(sim, 0.0, 1.0, out=sim)          # p_predict clamps to [0,1], predict/Predictor.cpp:293-298
        return close, sim

    def search_pairs(self, db, db_slots, qset, q_slots, win_lo=None, win_hi=None, m=None):
        """work() for every query of q_slots against the candidate list, the CLOSE pairs only (msc_search_pairs). Pair (q, i) is listed when
        win_lo[q] <= i < win_hi[q] (no windows: every i) and the classification block calls it close; its similarity is clamp(p_predict, 0, 1)
        (1 without a regression block). -> (offsets [n_q + 1] uint64, cand_idx uint32, sim float64, info): query q's pairs are
        [offsets[q], offsets[q + 1]) of cand_idx / sim, ascending i; info = dict(n_pairs, route (PAIRS_ROUTE_MATRIX / _FALLBACK), fp64_pairs)."""
        sl, m = _slots(db_slots, m)
        qs = np.ascontiguousarray(q_slots, dtype=np.uint32)
        nq = qs.size
        if (win_lo is None) != (win_hi is None):
            raise ValueError("win_lo and win_hi are given together or not at all")
        lo = None if win_lo is None else np.ascontiguousarray(win_lo, dtype=np.uint64)
        hi = None if win_hi is None else np.ascontiguousarray(win_hi, dtype=np.uint64)
        if lo is not None and (lo.size != nq or hi.size != nq):
            raise ValueError("one window per query")
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        info = _capi.PairsInfo()
        lib, h = self.ctx.lib, self.ctx.h
        self.ctx.check(lib.msc_search_pairs(h, self.cls.h if self.cls else None, self.reg.h if self.reg else None, db.h, _ptr(sl), m, qset.h, _ptr(qs), nq,
                                            _ptr(lo), _ptr(hi), _ptr(offsets), C.byref(info)))
        n = int(info.n_pairs)
        idx = np.zeros(max(n, 1), dtype=np.uint32)
        sim = np.zeros(max(n, 1))
        self.ctx.check(lib.msc_search_pairs_fetch(h, 0, n, _ptr(idx), _ptr(sim)))
        return offsets, idx[:n], sim[:n], dict(n_pairs=n, route=int(info.route), fp64_pairs=int(info.fp64_pairs))

    def search_pairs_top(self, db, db_slots, qset, q_slots, top, win_lo=None, win_hi=None, m=None):
        """search_pairs with each query's list cut to its `top` best pairs on the device (msc_search_pairs_top): all of a query's pairs where
        it has at most `top`, else the `top` of largest similarity (compared as doubles, ties to the lower candidate index), still in
        ascending candidate index and with the bits search_pairs returns; top = 0 is no cut. -> (offsets, cand_idx, sim, info) as
        search_pairs, info["close_counts"] (uint64 [n_q]) = each query's pairs before the cut."""
        sl, m = _slots(db_slots, m)
        qs = np.ascontiguousarray(q_slots, dtype=np.uint32)
        nq = qs.size
        top = int(top)
        if not 0 <= top <= 0xFFFFFFFF:
            raise ValueError("top is a 32-bit count")
        if (win_lo is None) != (win_hi is None):
            raise ValueError("win_lo and win_hi are given together or not at all")
        lo = None if win_lo is None else np.ascontiguousarray(win_lo, dtype=np.uint64)
        hi = None if win_hi is None else np.ascontiguousarray(win_hi, dtype=np.uint64)
        if lo is not None and (lo.size != nq or hi.size != nq):
            raise ValueError("one window per query")
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        counts = np.zeros(max(nq, 1), dtype=np.uint64)
        info = _capi.PairsInfo()
        lib, h = self.ctx.lib, self.ctx.h
        self.ctx.check(lib.msc_search_pairs_top(h, self.cls.h if self.cls else None, self.reg.h if self.reg else None, db.h, _ptr(sl), m, qset.h, _ptr(qs), nq,
                                                _ptr(lo), _ptr(hi), top, _ptr(offsets), _ptr(counts), C.byref(info)))
        n = int(info.n_pairs)
        idx = np.zeros(max(n, 1), dtype=np.uint32)
        sim = np.zeros(max(n, 1))
        self.ctx.check(lib.msc_search_pairs_fetch(h, 0, n, _ptr(idx), _ptr(sim)))
        return offsets, idx[:n], sim[:n], dict(n_pairs=n, route=int(info.route), fp64_pairs=int(info.fp64_pairs), close_counts=counts[:nq])

    def search_pairs_strands(self, db, db_slots, qset, q_slots, win_lo=None, win_hi=None, m=None):
        """search_pairs on both strands (msc_search_pairs_strands): per query the union, ascending candidate index, of its list and of the list of
        its reverse complement against the candidates as stored. A pair of both lists keeps the larger similarity (a tie goes to forward).
        -> (offsets, cand_idx, sim, strand uint8 (0 forward, 1 reverse), info) with info as search_pairs: fp64_pairs summed over both passes, route
        MATRIX iff both passes took it."""
        sl, m = _slots(db_slots, m)
        qs = np.ascontiguousarray(q_slots, dtype=np.uint32)
        nq = qs.size
        if (win_lo is None) != (win_hi is None):
            raise ValueError("win_lo and win_hi are given together or not at all")
        lo = None if win_lo is None else np.ascontiguousarray(win_lo, dtype=np.uint64)
        hi = None if win_hi is None else np.ascontiguousarray(win_hi, dtype=np.uint64)
        if lo is not None and (lo.size != nq or hi.size != nq):
            raise ValueError("one window per query")
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        info = _capi.PairsInfo()
        lib, h = self.ctx.lib, self.ctx.h
        self.ctx.check(lib.msc_search_pairs_strands(h, self.cls.h if self.cls else None, self.reg.h if self.reg else None, db.h, _ptr(sl), m, qset.h, _ptr(qs), nq,
                                                    _ptr(lo), _ptr(hi), _ptr(offsets), C.byref(info)))
        n = int(info.n_pairs)
        idx = np.zeros(max(n, 1), dtype=np.uint32)
        sim = np.zeros(max(n, 1))
        strand = np.zeros(max(n, 1), dtype=np.uint8)
        self.ctx.check(lib.msc_search_pairs_fetch(h, 0, n, _ptr(idx), _ptr(sim)))
        self.ctx.check(lib.msc_search_pairs_fetch_strands(h, 0, n, _ptr(strand)))
        return offsets, idx[:n], sim[:n], strand[:n], dict(n_pairs=n, route=int(info.route), fp64_pairs=int(info.fp64_pairs))
