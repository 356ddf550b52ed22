// msc_mirrors.hip -- the mirrors a histogram set carries beside its bins or lists for the Q x M calls (msc_score_multi, msc_search_pairs): the
// digest (pair_digest.hip), the presence bits with the lists of large bins and their folded form (msc_pair_gemm.hip, msc_fold.h), the ranks with
// their 16-bit form and moments (msc_emd_ranks.hip, msc_emd_list.hip). Each is built on first use and refreshed for the slots written since
// (ensure_*); here too: what marks them stale, what frees them, what they weigh in msc_hist_set_bytes, and the host-side bounds of the
// matrix-core pass that reads them. Split from msc_api_multi.hip and msc_api.hip.
#include <algorithm>
#include <cstdlib>

#include "msc_internal.h"
#include "msc_fold.h"
#include "msc_fold_reject.h"

#include "msc_objects.h"
#include "msc_api_private.h"

// every writer of slots ends here: the mirrors the set has (dense: digest, sparse lists, presence bits, ranks; sparse: presence bits,
// ranks) are stale for [first, first + n)
void mark_stale(msc_hist_set* s, uint64_t first, uint64_t n) {
	if (s->digest) s->dg_stale.add(first, n);
	if (s->sp_mirror) s->sm_stale.add(first, n);
	if (s->kb) s->kb_stale.add(first, n);
	if (s->ranks) s->rk_stale.add(first, n);
	if (s->rj_ranges) s->rj_stale.add(first, n);
}

// the presence bits, the lists of large bins and the folded form beside them: freed together (ensure_kb, when one of them cannot be had)
static void free_kb_mirror(const msc_hist_set* set) {
	if (set->kb) (void)hipFree(set->kb);
	if (set->mb) (void)hipFree(set->mb);
	if (set->mb_n) (void)hipFree(set->mb_n);
	if (set->kbf) (void)hipFree(set->kbf);
	if (set->kbf_x) (void)hipFree(set->kbf_x);
	set->kb = nullptr; set->mb = nullptr; set->mb_n = nullptr; set->kbf = nullptr; set->kbf_x = nullptr; set->kbf_fold = 0;
}

// every mirror of this file (the set is going away: nothing of it is in flight)
void free_mirrors(const msc_hist_set* set) {
	if (set->digest) (void)hipFree(set->digest);
	free_kb_mirror(set);
	if (set->ranks) (void)hipFree(set->ranks);
	if (set->ranks16) (void)hipFree(set->ranks16);
	if (set->rk_n) (void)hipFree(set->rk_n);
	if (set->rk_sum) (void)hipFree(set->rk_sum);          // (rk_dev is its second half)
	if (set->rj_ranges) (void)hipFree(set->rj_ranges);
	set->rj_ranges = nullptr;
	set->digest = nullptr; set->ranks = nullptr; set->ranks16 = nullptr; set->rk_n = nullptr; set->rk_sum = set->rk_dev = nullptr;
}

// What the mirrors add to a slot in msc_hist_set_bytes. (As it always counted: the 16-bit ranks of a sparse set only, and neither the folded
// mirror nor the moments.)
uint64_t mirror_bytes_per_slot(const msc_hist_set* s) {
	return (s->digest ? msc_digest_slot_bytes(s->L) : 0) + (s->kb ? s->L.padded_bins / 8 + 32 + (uint64_t)s->mb_pitch * 8 + 4 : 0) + (s->ranks ? (s->rk_pitch + 1) * 4 : 0) +
	       (s->sparse && s->ranks16 ? s->rk_pitch * 2 : 0);
}

// The digest mirror of a dense 32-bit set (pair_digest.hip): allocated on first use, refreshed for the slots written since.
// Returns MSC_OK with set->digest == nullptr when the mirror cannot be had (no memory): the caller then streams the raw bins.
int ensure_digest(msc_ctx* ctx, const msc_hist_set* set) {
	if (set->sparse || !msc_digest_supported(set->L) || set->digest_unavailable) return MSC_OK;
	if (!set->digest) {
		void* p = nullptr;
		if (hipMalloc(&p, msc_digest_slot_bytes(set->L) * set->capacity) != hipSuccess) {
			(void)hipGetLastError();
			set->digest_unavailable = true;
			return MSC_OK;
		}
		set->digest = (uint8_t*)p;
		set->dg_stale.all(set->capacity);
	}
	if (set->dg_stale.any()) {
		HIP_TRY(ctx, msc_launch_digest_build(ctx->stream, set->L, set->bins, set->scalars, set->digest, set->dg_stale.lo, set->dg_stale.hi - set->dg_stale.lo));
		set->dg_stale.clear();
	}
	return MSC_OK;
}

// The folded mirror beside kb (msc_fold.h), for the fold the context asks for: set-up work on a resident set, done once and refreshed with kb.
// Without memory for it the set is simply not folded. (ensure_kb calls it for the calls the folded screen serves -- msc_search_pairs builds none.)
static int ensure_kb_folded(msc_ctx* ctx, const msc_hist_set* set) {
	const uint32_t fold = msc_fold_fits(set->L, ctx->fold_screen) ? ctx->fold_screen : 0;
	if (set->kbf && set->kbf_fold != fold) {
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		(void)hipFree(set->kbf); (void)hipFree(set->kbf_x);
		set->kbf = nullptr; set->kbf_x = nullptr; set->kbf_fold = 0;
	}
	if (fold && !set->kbf) {
		MscLayout Lf = set->L;
		Lf.padded_bins = Lf.nbins = set->L.nbins / fold;
		void *p = nullptr, *px = nullptr;
		if (hipMalloc(&p, msc_kb_bytes(Lf, set->capacity)) != hipSuccess || hipMalloc(&px, (set->capacity + 31) / 32 * 32 * sizeof(uint32_t)) != hipSuccess) {
			(void)hipGetLastError();
			if (p) (void)hipFree(p);
			return MSC_OK;
		}
		set->kbf = (uint8_t*)p; set->kbf_x = (uint32_t*)px; set->kbf_fold = fold;
		set->kbf_stale.all(set->capacity);
	}
	if (set->kbf && set->kbf_stale.any()) {
		HIP_TRY(ctx, msc_launch_kb_fold(ctx->stream, set->L.nbins, fold, set->kb, set->kbf, set->kbf_x, set->kbf_stale.lo, set->kbf_stale.hi - set->kbf_stale.lo));
		set->kbf_stale.clear();
	}
	return MSC_OK;
}

// The presence-bit mirror of a set and its lists of large bins (msc_pair_gemm.hip): the operands of the int8 product that takes the
// Q x M pass. A dense set's come from its bins, a sparse set's from its entry lists (the same bytes for the same sequences; every slot of
// the stale range is rebuilt, a slot without a list as an all-zero image). MSC_OK with set->kb == nullptr when it cannot be had (no
// memory): the older routes then run.
int ensure_kb(msc_ctx* ctx, const msc_hist_set* set, bool want_fold) {
	if (set->kb_unavailable || set->dtype == 64) return MSC_OK;
	auto give_up = [&] {
		(void)hipGetLastError();
		free_kb_mirror(set);
		set->kb_unavailable = true;
		return MSC_OK;
	};
	if (!set->kb) {
		void *p = nullptr, *pm = nullptr, *pn = nullptr;
		set->mb_pitch = 16;
		if (hipMalloc(&p, msc_kb_bytes(set->L, set->capacity)) != hipSuccess) return give_up();
		set->kb = (uint8_t*)p;
		if (hipMalloc(&pm, (size_t)set->capacity * set->mb_pitch * 8) != hipSuccess) return give_up();
		set->mb = pm;
		if (hipMalloc(&pn, (size_t)set->capacity * 4) != hipSuccess) return give_up();
		set->mb_n = (uint32_t*)pn;
		HIP_TRY(ctx, hipMemsetAsync(set->mb_n, 0, (size_t)set->capacity * 4, ctx->stream));
		set->mb_n_host.assign(set->capacity, 0);
		set->kb_stale.all(set->capacity);
	}
	auto written = [&](uint64_t i) { return set->written[i] != 0; };
	while (set->kb_stale.any()) {
		// runs of slots that hold a histogram; the build reports a zero count (sticky: the pass's identities take count - 1 of every
		// bin) and the longest list of large bins it met: past the pitch, the lists are laid out again and every written slot rebuilt
		int r;
		if ((r = ensure(ctx, ctx->rk_bad, 2 * sizeof(int32_t)))) return r;
		HIP_TRY(ctx, hipMemsetAsync(ctx->rk_bad.p, 0, 2 * sizeof(int32_t), ctx->stream));
		const uint64_t lo = set->kb_stale.lo, hi = std::min<uint64_t>(set->kb_stale.hi, set->sparse ? set->capacity : set->written.size());
		if (set->sparse) {          // every slot of the range: one without a list gets an all-zero image and an empty list
			if (hi > lo) HIP_TRY(ctx, msc_launch_kb_build_sparse(ctx->stream, set->L, set->ent, set->hdr, set->kb, lo, hi - lo, set->mb, set->mb_n, set->mb_pitch, (int32_t*)ctx->rk_bad.p));
		} else if ((r = for_each_run(lo, hi, written, [&](uint64_t first, uint64_t n) {
			            HIP_TRY(ctx, msc_launch_kb_build(ctx->stream, set->L, set->dtype, set->bins, set->kb, first, n, set->mb, set->mb_n, set->mb_pitch, (int32_t*)ctx->rk_bad.p));
			            return (int)MSC_OK;
		            })))
			return r;
		int32_t flags[2] = {0, 0};
		HIP_TRY(ctx, hipMemcpyAsync(flags, ctx->rk_bad.p, sizeof flags, hipMemcpyDeviceToHost, ctx->stream));
		if (hi > lo) HIP_TRY(ctx, hipMemcpyAsync(set->mb_n_host.data() + lo, set->mb_n + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		if (flags[0]) set->kb_has_zero = true;
		if (set->kbf) set->kbf_stale.add(lo, hi > lo ? hi - lo : 0);          // (invalidated wherever kb is)
		set->kb_stale.clear();
		if ((uint32_t)flags[1] > set->mb_pitch) {
			const uint32_t pitch = ((uint32_t)flags[1] + 15) / 16 * 16;
			void* pm = nullptr;
			(void)hipFree(set->mb);
			set->mb = nullptr;
			if (hipMalloc(&pm, (size_t)set->capacity * pitch * 8) != hipSuccess) return give_up();
			set->mb = pm;
			set->mb_pitch = pitch;
			set->kb_stale.all(set->capacity);
		}
	}
	return want_fold && set->kb ? ensure_kb_folded(ctx, set) : (int)MSC_OK;
}

// The ranks mirror of a set (msc_emd_ranks.hip), from a dense set's bins or a sparse set's lists. MSC_OK with set->ranks == nullptr when
// it cannot be had (no memory, or a slot holds a zero count): the digest kernel then keeps the prefixes.
int ensure_ranks(msc_ctx* ctx, const msc_hist_set* set) {
	if (set->dtype == 64 || !msc_digest_supported(set->L) || set->ranks_unavailable || set->max_sum < set->L.nbins) return MSC_OK;
	const uint64_t pitch = msc_ranks_pitch(set->max_sum - set->L.nbins);
	if (set->ranks && pitch > set->rk_pitch) {          // a longer list than any before: lay the mirror out again
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		(void)hipFree(set->ranks);
		set->ranks = nullptr;
		if (set->ranks16) { (void)hipFree(set->ranks16); set->ranks16 = nullptr; }
		set->rk16_off = false;
	}
	if (!set->ranks) {
		void *p = nullptr, *pn = set->rk_n;
		if (hipMalloc(&p, pitch * 4 * set->capacity) != hipSuccess || (!pn && hipMalloc(&pn, 4 * set->capacity) != hipSuccess)) {
			(void)hipGetLastError();
			if (p) (void)hipFree(p);
			set->ranks_unavailable = true;
			return MSC_OK;
		}
		set->ranks = (uint32_t*)p;
		set->rk_n = (uint32_t*)pn;
		set->rk_pitch = pitch;
		set->rk_stale.all(set->capacity);
		if (set->rj_ranges) set->rj_stale.all(set->capacity);          // (every slot's moment is taken again at the new pitch: the ranges behind the cut start over)
		if (!set->rk_sum) {          // the two moments per slot (msc_emd_list.hip), built with the rows below; without them the close flags take the dense walk
			void* pm = nullptr;
			if (hipMalloc(&pm, 2 * sizeof(uint64_t) * set->capacity) != hipSuccess) (void)hipGetLastError();
			else { set->rk_sum = (uint64_t*)pm; set->rk_dev = set->rk_sum + set->capacity; }
		}
	}
	static const bool no_rk16 = getenv("MSC_NO_RANKS16") != nullptr;
	if (!set->ranks16 && !set->rk16_off && !no_rk16 && set->rk_pitch % 1024 == 0) {          // the 16-bit form beside it (k_emd_ranks16)
		void* p16 = nullptr;
		if (hipMalloc(&p16, set->rk_pitch * 2 * set->capacity) != hipSuccess) { (void)hipGetLastError(); set->rk16_off = true; }
		else { set->ranks16 = (uint16_t*)p16; set->rk_stale.all(set->capacity); }
	}
	if (set->rk_stale.any()) {
		int r;
		if ((r = ensure(ctx, ctx->rk_bad, 2 * sizeof(int32_t)))) return r;
		HIP_TRY(ctx, hipMemsetAsync(ctx->rk_bad.p, 0, 2 * sizeof(int32_t), ctx->stream));
		// runs of slots that hold a histogram (an unwritten slot's digest is whatever the allocation held)
		const uint64_t lo = set->rk_stale.lo, hi = std::min<uint64_t>(set->rk_stale.hi, set->sparse ? set->capacity : set->written.size());
		int32_t* bad_word = (int32_t*)ctx->rk_bad.p;
		auto build16 = [&](uint64_t first, uint64_t n) {          // (a dense set: and the moments of the same rows, msc_emd_list.hip)
			if (set->rk_sum && !set->sparse) HIP_TRY(ctx, msc_launch_rank_moments(ctx->stream, set->L.nbins, set->ranks, set->rk_pitch, first, n, set->rk_sum, set->rk_dev));
			if (set->ranks16) HIP_TRY(ctx, msc_launch_ranks16_build(ctx->stream, set->L.nbins, set->ranks, set->ranks16, set->rk_pitch, first, n, bad_word + 1));
			return (int)MSC_OK;
		};
		if (set->sparse) {
			// the 32-bit ranks of every slot of the range from its list (one without a list: all padding, n = 0); the 16-bit form only of the
			// runs that hold a list, as a dense set's unwritten slots are skipped: the ranks16 row of an empty slot is NOT maintained (all
			// padding does not fit 16 bits and would switch the form off for the set; nothing reads a row past its rk_n = 0)
			if (hi > lo) HIP_TRY(ctx, msc_launch_ranks_build_sparse(ctx->stream, set->L, set->ent, set->cum, set->hdr, set->ranks, set->rk_n, set->rk_pitch, lo, hi - lo, bad_word));
			if (hi > lo && set->rk_sum) HIP_TRY(ctx, msc_launch_rank_moments(ctx->stream, set->L.nbins, set->ranks, set->rk_pitch, lo, hi - lo, set->rk_sum, set->rk_dev));
			if ((r = for_each_run(lo, hi, [&](uint64_t i) { return set->hdr_host[i].nnz != 0; }, build16))) return r;
		} else if ((r = for_each_run(lo, hi, [&](uint64_t i) { return set->written[i] != 0; }, [&](uint64_t first, uint64_t n) {
			            HIP_TRY(ctx, msc_launch_ranks_build(ctx->stream, set->L, set->dtype, set->bins, set->scalars, set->ranks, set->rk_n, set->rk_pitch, first, n, bad_word));
			            return build16(first, n);
		            })))
			return r;
		int32_t bad[2] = {0, 0};
		HIP_TRY(ctx, hipMemcpyAsync(bad, ctx->rk_bad.p, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		set->rk_stale.clear();
		if (bad[0]) {
			(void)hipFree(set->ranks);
			set->ranks = nullptr;
			set->ranks_unavailable = true;
		}
		if ((bad[0] || bad[1]) && set->ranks16) {          // a reduced rank that does not fit 16 bits: this set keeps the 32-bit walk
			(void)hipFree(set->ranks16);
			set->ranks16 = nullptr;
			set->rk16_off = true;
		}
	}
	return MSC_OK;
}

// The ranges the cut of a folded block reads of its candidates (msc_fold_reject.h): minima and maxima of the scalar records' four, the largest second rank
// moment and the largest sum of (e - 1) over a list of large bins, over the slots that hold a histogram -- beside the mirrors they are read from (the lists of
// ensure_kb, the moments of ensure_ranks: both stand when this is called), once per range of slots written since. A slot written again adds its new values
// to the ranges and its old ones stay: wider ranges certify less and never wrongly -- for the values of ONE ranks pitch. The moments depend on the pitch, so
// when ensure_ranks lays the mirror out again it marks every slot stale here, and a stale range that covers the whole set starts the ranges from empty (which
// also lets a set that once held an outlier have its cuts back after a full rewrite). MSC_OK with set->rj_ranges == nullptr when they cannot be had.
int ensure_reject_ranges(msc_ctx* ctx, const msc_hist_set* set) {
	if (!set->mb || !set->mb_n || !set->rk_dev) return MSC_OK;
	if (!set->rj_ranges) {
		void* p = nullptr;
		if (hipMalloc(&p, sizeof(MscRejectRanges)) != hipSuccess) { (void)hipGetLastError(); return MSC_OK; }
		set->rj_ranges = (uint64_t*)p;
		set->rj_stale.all(set->capacity);
	}
	if (set->rj_stale.any()) {
		if (set->rj_stale.lo == 0 && set->rj_stale.hi >= set->capacity) {
			static const MscRejectRanges empty{~0ull, 0, ~0ull, 0, ~0ull, 0, ~0ull, 0, 0, 0};
			HIP_TRY(ctx, hipMemcpyAsync(set->rj_ranges, &empty, sizeof empty, hipMemcpyHostToDevice, ctx->stream));
		}
		const uint64_t lo = set->rj_stale.lo, hi = std::min<uint64_t>(set->rj_stale.hi, set->sparse ? set->hdr_host.size() : set->written.size());
		const int r = for_each_run(lo, hi, [&](uint64_t i) { return set->sparse ? set->hdr_host[i].nnz != 0 : set->written[i] != 0; }, [&](uint64_t first, uint64_t n) {
			HIP_TRY(ctx, msc_launch_fold_reject_ranges(ctx->stream, set->scalars, set->scalar_stride, set->mb, set->mb_n, set->mb_pitch, set->rk_dev, first, n, set->rj_ranges));
			return (int)MSC_OK;
		});
		if (r) return r;
		set->rj_stale.clear();
	}
	return MSC_OK;
}

// whether every one of the m candidates of a call (slots, or 0 .. m - 1) holds a histogram: the ranges above cover no other slot
bool reject_ranges_cover(const msc_hist_set* set, const uint32_t* slots, uint64_t m) {
	if (!set->sparse && !slots) {          // slots 0 .. m - 1 of a dense set: the leading run of written slots only grows, so it is walked once
		while (set->written_run < set->written.size() && set->written[set->written_run]) set->written_run++;
		return m <= set->written_run;
	}
	auto holds = [&](uint64_t i) { return set->sparse ? i < set->hdr_host.size() && set->hdr_host[i].nnz != 0 : i < set->written.size() && set->written[i] != 0; };
	for (uint64_t i = 0; i < m; i++) if (!holds(slots ? slots[i] : i)) return false;
	return true;
}

// Whether the pass on the matrix cores (msc_pair_gemm.hip) can take a Q x M call over these sets -- host-side bounds only: dense 8/16/32-bit
// sets of the narrow range whose histograms are whole 4 KiB tiles, P1 / P2 within int32 and, when
// the earth mover's distance is wanted, lists short enough for the ranks mirror (msc_emd_ranks.hip). Two sparse sets under the same
// bounds with msc_set_sparse_matrix_pass on, up to 2^20 bins (their mirrors come from the lists); never one of each.
bool kb_route_fits(const msc_hist_set* cands, const msc_hist_set* qset, bool need_emd) {
	static const bool off = getenv("MSC_MULTI_NO_GEMM") != nullptr;
	static const bool no_ranks = getenv("MSC_MULTI_NO_RANKS") != nullptr;
	const MscLayout& L = cands->L;
	if (cands->sparse != qset->sparse || (cands->sparse && (!cands->ctx->sparse_matrix_pass || L.nbins > (1ull << 20)))) return false;
	// (what msc_launch_kb_build_sparse asks of the layout, so that a set it cannot serve stays on the list passes instead of failing the call)
	if (cands->sparse && !msc_kb_build_sparse_fits(L)) return false;
	if (off || cands->dtype == 64 || L.nbins != L.padded_bins || !msc_digest_supported(L) || needs_wide(cands, qset)) return false;
	const uint64_t ms_ = std::max(cands->max_sum, qset->max_sum);
	if (ms_ < L.nbins || ms_ - L.nbins >= (1ull << 24)) return false;          // (P1 <= the k-mers of either sequence is summed in f32: exact below 2^24; the corrections stay within int32)
	if (need_emd && (no_ranks || L.nbins > (1ull << 20) || (ms_ - L.nbins) * 4 > L.nbins)) return false;
	return true;
}
