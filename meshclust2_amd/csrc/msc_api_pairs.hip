// msc_api_pairs.hip -- msc_search_pairs: fastcar's work() (fastcar/FC_Runner.cpp:426-471) for many queries, with the close pairs and their
// similarity as the only output. Two routes:
//   matrix   -- msc_score_multi's pass on the matrix cores (msc_pair_gemm.hip) per block of up to 128 queries, the classification flags left on
//               the device, then the list kernels of pair_features.hip (k_pair_list_count / _scan / _write): the regression model is
//               evaluated in FP64 for the listed pairs only, and nothing of size n_q x m crosses to the host. A model that holds
//               jefferey_divergence or jensen_shannon takes it only with msc_set_pairs_div_cells: the two sums then come from (count, count)
//               cells (k_pair_epilogue_bits_div) and agree with the fallback's to rounding, not bit for bit.
//   fallback -- every other case: msc_score_multi one block of queries at a time (dense flags and sums of that block on the host), compacted
//               there and copied up, so that msc_search_pairs_fetch reads one list whichever route ran.
// msc_search_pairs_top is the same body with a cut behind each block's list: the block's pairs go to the staging list on either route, and
// k_pair_top_plan / k_pair_top_select (pair_features.hip) write each query's top_n best from there to the call's list.
// msc_search_pairs_strands is the body twice -- the queries as given, then their reverse complements (msc_hist_revcomp_batch into a scratch set of
// the context) -- and a merge of the two lists on the device (k_pair_strand_count / _scan / _write).
#include <algorithm>
#include <cstring>
#include <vector>

#include "msc_internal.h"

#include "msc_objects.h"
#include "msc_api_private.h"

namespace {

struct PairsBlock {
	uint64_t q0, nq;          // queries [q0, q0 + nq)
	uint64_t lo, hi;          // the union of their windows: the candidates the block is evaluated over
};

// the list (idx, sim) holds `keep` pairs; make room for `need`
int grow_list(msc_ctx* ctx, DevBuf& idx, DevBuf& sim, uint64_t keep, uint64_t need) {
	if (need * sizeof(double) <= sim.cap && need * sizeof(uint32_t) <= idx.cap) return MSC_OK;
	const uint64_t n = std::max<uint64_t>(std::max<uint64_t>(need, sim.cap / sizeof(double) * 3 / 2), 4096);
	void *pi = nullptr, *ps = nullptr;
	if (hipMalloc(&pi, n * sizeof(uint32_t)) != hipSuccess || hipMalloc(&ps, n * sizeof(double)) != hipSuccess) {
		(void)hipGetLastError();
		if (pi) (void)hipFree(pi);
		return fail(ctx, MSC_ERR_OOM, "msc_search_pairs: no device memory for a list of %llu pairs", (unsigned long long)need);
	}
	if (keep) {
		HIP_TRY(ctx, hipMemcpyAsync(pi, idx.p, keep * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ps, sim.p, keep * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	release(idx);
	release(sim);
	idx.p = pi; idx.cap = n * sizeof(uint32_t);
	sim.p = ps; sim.cap = n * sizeof(double);
	return MSC_OK;
}

// a 64-bit word of the device read back (the stream is waited for)
int read_word(msc_ctx* ctx, const uint64_t* d, uint64_t* out) {
	int r;
	if ((r = ensure_pinned(ctx, ctx->pl_pin, 64))) return r;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->pl_pin.p, d, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	*out = *(const uint64_t*)ctx->pl_pin.p;
	return MSC_OK;
}

struct PairsCall {
	msc_ctx* ctx;
	const msc_model *cls, *reg;
	const msc_hist_set* cands;
	const uint32_t* cand_slots;
	uint64_t m;
	const msc_hist_set* qset;
	const uint32_t* q_slots;
	uint64_t n_q;
	bool windows;
	std::vector<uint64_t> win;          // [0, n_q): lo, [n_q, 2 n_q): hi (clamped to m, lo <= hi)
	std::vector<PairsBlock> blocks;
	std::vector<uint64_t> qcount;       // pairs per query
	uint64_t fp64 = 0;
	bool need_emd = false;
	bool cls_div = false, reg_div = false;          // msc_set_pairs_div_cells: the model holds a divergence statistic, its sums come from cells
	uint32_t top_n = 0;                 // msc_search_pairs_top: pairs kept per query (0 = all; qcount stays the count before the cut)
};

// the cut of a block whose pairs lie in the staging list as pl_seg says ([n_chunks][nb] of {first, n}): the list grows from `total` by
// the kept pairs, known once the plan kernel has run, and the selection writes them to their final places
int cut_block(msc_ctx* ctx, uint32_t n_chunks, uint32_t nb, uint32_t top_n, uint64_t& total) {
	int r;
	uint64_t* words = (uint64_t*)ctx->pl_words.p;
	HIP_TRY(ctx, msc_launch_pair_top_plan(ctx->stream, (const uint64_t*)ctx->pl_seg.p, n_chunks, nb, top_n, words, (uint64_t*)ctx->pl_dst.p));
	uint64_t now = 0;
	if ((r = read_word(ctx, words, &now))) return r;
	if ((r = grow_list(ctx, ctx->pl_idx, ctx->pl_sim, total, now))) return r;
	HIP_TRY(ctx, msc_launch_pair_top_select(ctx->stream, (const uint64_t*)ctx->pl_seg.p, n_chunks, nb, top_n, (const uint64_t*)ctx->pl_dst.p, (const uint32_t*)ctx->pl_stage_idx.p,
	                                        (const double*)ctx->pl_stage_sim.p, (uint32_t*)ctx->pl_idx.p, (double*)ctx->pl_sim.p));
	total = now;
	return MSC_OK;
}

// blocks of up to blk queries (none of one query when there are more: the product pass takes two and up), each with its union window;
// a block whose members' windows are all empty is left out
void plan_blocks(PairsCall& c, uint64_t blk) {
	c.blocks.clear();
	for (uint64_t q0 = 0; q0 < c.n_q;) {
		uint64_t nq = std::min(blk, c.n_q - q0);
		if (c.n_q - q0 - nq == 1 && nq > 2) nq--;
		PairsBlock b{q0, nq, 0, c.m};
		if (c.windows) {
			b.lo = c.m; b.hi = 0;
			for (uint64_t q = q0; q < q0 + nq; q++)
				if (c.win[q] < c.win[c.n_q + q]) { b.lo = std::min(b.lo, c.win[q]); b.hi = std::max(b.hi, c.win[c.n_q + q]); }
		}
		if (b.lo < b.hi) c.blocks.push_back(b);
		q0 += nq;
	}
}

int run_matrix(PairsCall& c) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	const MscLayout& L = cands->L;
	hipStream_t st = ctx->stream;
	const uint64_t n_q = c.n_q;
	int r;
	// the call's query slots, windows, per-query counts and running totals {list, staging list, pairs the screen left open}
	if ((r = ensure(ctx, ctx->pl_qslots, n_q * sizeof(uint32_t))) || (r = ensure(ctx, ctx->pl_qcount, n_q * sizeof(uint64_t))) ||
	    (r = ensure(ctx, ctx->pl_words, 4 * sizeof(uint64_t))) || (r = ensure(ctx, ctx->err_word, sizeof(int32_t))))
		return r;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->pl_qslots.p, c.q_slots, n_q * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemsetAsync(ctx->pl_qcount.p, 0, n_q * sizeof(uint64_t), st));
	HIP_TRY(ctx, hipMemsetAsync(ctx->pl_words.p, 0, 4 * sizeof(uint64_t), st));
	HIP_TRY(ctx, hipMemsetAsync(ctx->err_word.p, 0, sizeof(int32_t), st));
	if (c.windows) {
		if ((r = ensure(ctx, ctx->pl_win, 2 * n_q * sizeof(uint64_t)))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->pl_win.p, c.win.data(), 2 * n_q * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	}
	if (c.cand_slots) {
		if ((r = ensure(ctx, ctx->slots, c.m * sizeof(uint32_t)))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->slots.p, c.cand_slots, c.m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	}
	uint64_t* words = (uint64_t*)ctx->pl_words.p;
	uint64_t total = 0;          // pairs in the list so far
	uint64_t uncut = 0;          // msc_search_pairs_top: pairs listed before the cut
	const bool cut = c.top_n != 0;
	const bool screen = c.cls && c.cls->h.screen_ok;
	uint32_t last_qn = 0;
	BlockPipe::Side& side = ctx->pipe.side[0];
	for (const PairsBlock& b : c.blocks) {
		const uint32_t nb = (uint32_t)b.nq;
		const uint64_t mall = b.hi - b.lo;
		const uint32_t kb_qn = msc_pair_gemm_rows(nb);
		last_qn = kb_qn;
		const uint64_t n_hot = block_hot_size(qset, c.q_slots + b.q0, nb);
		const MscCandChunks cc = matrix_chunks(ctx, L.nbins, mall, kb_qn);          // candidate chunks as msc_score_multi cuts them
		const uint64_t chunk = cc.chunk;
		const uint32_t n_chunks = (uint32_t)cc.n;
		const bool stage = n_chunks > 1 || cut;          // the block's pairs go to the staging list first
		const uint32_t slices = msc_pair_gemm_slices(L.nbins, (uint32_t)chunk, kb_qn, ctx->num_cus);
		const uint32_t tiles = msc_pair_list_tiles((uint32_t)chunk);
		HotList hot;
		if ((r = ensure_side(ctx, side, L.nbins, kb_qn, slices, chunk, n_hot, &hot)) || (r = ensure(ctx, ctx->pl_counts, (size_t)nb * tiles * sizeof(uint32_t))) ||
		    (r = ensure(ctx, ctx->pl_offsets, ((size_t)nb * tiles + 1) * sizeof(uint64_t))))
			return r;
		if (c.need_emd && (r = ensure(ctx, ctx->emd_out, chunk * kb_qn * sizeof(uint64_t)))) return r;
		if (c.cls && (r = ensure(ctx, ctx->pl_flags, (size_t)nb * chunk))) return r;
		if (stage) {
			if ((r = ensure(ctx, ctx->pl_seg, (size_t)n_chunks * nb * 2 * sizeof(uint64_t))) || (r = ensure(ctx, ctx->pl_dst, (size_t)n_chunks * nb * sizeof(uint64_t)))) return r;
			HIP_TRY(ctx, hipMemsetAsync(words + 1, 0, sizeof(uint64_t), st));
		}
		const uint32_t* dq = (const uint32_t*)ctx->pl_qslots.p + b.q0;
		const uint64_t* dwl = c.windows ? (const uint64_t*)ctx->pl_win.p + b.q0 : nullptr;
		const uint64_t* dwh = c.windows ? (const uint64_t*)ctx->pl_win.p + n_q + b.q0 : nullptr;
		uint8_t* flags = c.cls ? (uint8_t*)ctx->pl_flags.p : nullptr;
		// the queries' side of the block, once for all chunks of candidates
		HIP_TRY(ctx, msc_launch_pair_gemm_queries(st, L.nbins, qset->kb, qset->mb, qset->mb_n, qset->mb_pitch, dq, nb, kb_qn, (uint8_t*)side.qT.p, n_hot, side.hot.p,
		                                          hot.ptr, hot.cursor, hot.cnt, (uint8_t*)side.anib.p));
		uint64_t staged = 0;
		uint32_t ci = 0;
		for (uint64_t off = b.lo; off < b.hi; off += chunk, ci++) {
			const uint32_t mc = (uint32_t)std::min(chunk, b.hi - off);
			const uint32_t* d_slots = c.cand_slots ? (const uint32_t*)ctx->slots.p + off : nullptr;
			HIP_TRY(ctx, msc_launch_pair_gemm(st, L.nbins, cands->kb, d_slots, off, mc, kb_qn, slices, hot.ptr, side.hot.p, (int32_t*)side.min.p, (int32_t*)side.diff.p,
			                                  (const uint8_t*)side.anib.p));
			if (c.need_emd) HIP_TRY(ctx, launch_emd_ranks(st, cands, qset, d_slots, off, mc, dq, nb, (uint64_t*)ctx->emd_out.p, kb_qn));
			MscEpilogueArgs ea;
			fill_pair_args(ea, ctx, cands, qset, d_slots, c.cand_slots ? 0 : off, mc, dq, c.q_slots[b.q0], nb, slices, MSC_ORDER_CAND_FIRST);
			fill_matrix_args(ea, side, cands, qset, slices, kb_qn, c.cand_slots ? 0 : off, n_hot, c.need_emd ? ctx->emd_out.p : nullptr);
			ea.kb_c_bits = cands->kb;
			if (c.cls) {          // the flags, as msc_score_multi decides them, kept here
				ea.model = c.cls->d;
				ea.close_soa = flags;
				ea.screen = screen && !c.cls_div;
				ea.div_cells = c.cls_div;
				HIP_TRY(ctx, msc_launch_pair_list_flags(st, ea, (unsigned long long*)(words + 2)));
				if (!ea.screen) c.fp64 += (uint64_t)nb * mc;
			}
			HIP_TRY(ctx, msc_launch_pair_list_count(st, flags, nb, mc, off, dwl, dwh, (uint32_t*)ctx->pl_counts.p));
			uint64_t* base = stage ? words + 1 : words;
			HIP_TRY(ctx, msc_launch_pair_list_scan(st, (const uint32_t*)ctx->pl_counts.p, nb, msc_pair_list_tiles(mc), base, (uint64_t*)ctx->pl_offsets.p,
			                                       (uint64_t*)ctx->pl_qcount.p + b.q0, stage ? (uint64_t*)ctx->pl_seg.p + (uint64_t)ci * nb * 2 : nullptr));
			uint64_t now = 0;
			if ((r = read_word(ctx, base, &now))) return r;          // the list grows before the write: no block runs past its end
			DevBuf& out_idx = stage ? ctx->pl_stage_idx : ctx->pl_idx;
			DevBuf& out_sim = stage ? ctx->pl_stage_sim : ctx->pl_sim;
			if ((r = grow_list(ctx, out_idx, out_sim, stage ? staged : total, now))) return r;
			if (stage) staged = now; else total = now;
			ea.model = c.reg ? c.reg->d : nullptr;
			ea.close_soa = nullptr;
			ea.screen = 0;
			ea.div_cells = c.reg_div;
			HIP_TRY(ctx, msc_launch_pair_list_write(st, ea, flags, off, dwl, dwh, (const uint64_t*)ctx->pl_offsets.p, (uint32_t*)out_idx.p, (double*)out_sim.p));
		}
		if (cut) {          // each query's best pairs out of the staged ones, into the list
			uncut += staged;
			if ((r = cut_block(ctx, n_chunks, nb, c.top_n, total))) return r;
		} else if (stage) {          // the block's chunks were staged chunk by chunk: into the list query by query
			if ((r = grow_list(ctx, ctx->pl_idx, ctx->pl_sim, total, total + staged))) return r;
			HIP_TRY(ctx, msc_launch_pair_list_gather(st, (const uint64_t*)ctx->pl_seg.p, n_chunks, nb, words, (uint64_t*)ctx->pl_dst.p, (const uint32_t*)ctx->pl_stage_idx.p,
			                                         (const double*)ctx->pl_stage_sim.p, (uint32_t*)ctx->pl_idx.p, (double*)ctx->pl_sim.p));
			total += staged;
		}
	}
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if ((r = read_error_word(ctx))) return r;
	HIP_TRY(ctx, hipMemcpy(c.qcount.data(), ctx->pl_qcount.p, n_q * sizeof(uint64_t), hipMemcpyDeviceToHost));
	uint64_t open = 0;
	if ((r = read_word(ctx, words + 2, &open))) return r;
	c.fp64 += open + (c.reg ? (cut ? uncut : total) : 0);
	ctx->pl_n = total;
	if (last_qn) {          // msc_last_kernel_info names the product kernel, as msc_score_multi does
		name_matrix_kernel(ctx, last_qn, c.need_emd, c.cls_div || c.reg_div, cands->sparse);
		ctx->last_query_tile = (int)c.blocks.back().nq;
		ctx->have_timing = false;
	}
	return MSC_OK;
}

int run_fallback(PairsCall& c) {
	msc_ctx* ctx = c.ctx;
	int r;
	std::vector<uint32_t> idx;
	std::vector<double> sim;
	std::vector<uint8_t> bclose;
	std::vector<double> bsim;
	std::vector<uint32_t> ids;
	const bool cut = c.top_n != 0;
	uint64_t total = 0;          // msc_search_pairs_top: pairs in the list so far
	std::vector<uint64_t> seg;
	if (cut) {
		if ((r = ensure(ctx, ctx->pl_words, 4 * sizeof(uint64_t)))) return r;
		HIP_TRY(ctx, hipMemsetAsync(ctx->pl_words.p, 0, 4 * sizeof(uint64_t), ctx->stream));
	}
	for (const PairsBlock& b : c.blocks) {
		const uint64_t mw = b.hi - b.lo;
		const uint32_t* sl = c.cand_slots ? c.cand_slots + b.lo : nullptr;
		if (!c.cand_slots && b.lo) {          // (the candidates [lo, hi) of the set: a slot list of them)
			ids.resize(mw);
			for (uint64_t i = 0; i < mw; i++) ids[i] = (uint32_t)(b.lo + i);
			sl = ids.data();
		}
		bclose.assign(b.nq * mw, 1);
		bsim.assign(b.nq * mw, 1.0);
		if (c.cls) {
			if ((r = msc_score_multi(ctx, c.cls, c.cands, sl, mw, c.qset, c.q_slots + b.q0, b.nq, MSC_ORDER_CAND_FIRST, nullptr, nullptr, bclose.data(), 0, nullptr))) return r;
			c.fp64 += b.nq * mw;
		}
		if (c.reg) {
			if ((r = msc_score_multi(ctx, c.reg, c.cands, sl, mw, c.qset, c.q_slots + b.q0, b.nq, MSC_ORDER_CAND_FIRST, bsim.data(), nullptr, nullptr, 0, nullptr))) return r;
			c.fp64 += b.nq * mw;
			for (double& v : bsim) v = v < 0 ? 0 : (v > 1 ? 1 : v);      // p_predict clamps to [0,1], predict/Predictor.cpp:293-298
		}
		if (cut) seg.assign(2 * b.nq, 0);
		for (uint64_t j = 0; j < b.nq; j++) {
			const uint64_t q = b.q0 + j;
			const uint64_t lo = c.windows ? c.win[q] : 0, hi = c.windows ? c.win[c.n_q + q] : c.m;
			if (cut) seg[2 * j] = idx.size();
			for (uint64_t i = lo; i < hi; i++) {
				const uint64_t at = j * mw + (i - b.lo);
				if (!bclose[at]) continue;
				idx.push_back((uint32_t)i);
				sim.push_back(bsim[at]);
				c.qcount[q]++;
			}
			if (cut) seg[2 * j + 1] = idx.size() - seg[2 * j];
		}
		if (cut && !idx.empty()) {          // the block's pairs up to the staging list, and the kernels of the matrix route cut them
			if ((r = ensure(ctx, ctx->pl_seg, seg.size() * sizeof(uint64_t))) || (r = ensure(ctx, ctx->pl_dst, b.nq * sizeof(uint64_t))) ||
			    (r = grow_list(ctx, ctx->pl_stage_idx, ctx->pl_stage_sim, 0, idx.size())))
				return r;
			HIP_TRY(ctx, hipMemcpyAsync(ctx->pl_seg.p, seg.data(), seg.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
			HIP_TRY(ctx, hipMemcpyAsync(ctx->pl_stage_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
			HIP_TRY(ctx, hipMemcpyAsync(ctx->pl_stage_sim.p, sim.data(), sim.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
			if ((r = cut_block(ctx, 1, (uint32_t)b.nq, c.top_n, total))) return r;
			HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (the vectors are reused by the next block)
			idx.clear();
			sim.clear();
		}
	}
	if (cut) {
		ctx->pl_n = total;
		return MSC_OK;
	}
	if ((r = grow_list(ctx, ctx->pl_idx, ctx->pl_sim, 0, idx.size()))) return r;
	if (!idx.empty()) {
		HIP_TRY(ctx, hipMemcpyAsync(ctx->pl_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->pl_sim.p, sim.data(), sim.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	ctx->pl_n = idx.size();
	return MSC_OK;
}

// msc_search_pairs (top_n = 0, close_counts = NULL) and msc_search_pairs_top
int search_pairs(msc_ctx* ctx, const msc_model* cls, const msc_model* reg, const msc_hist_set* db, const uint32_t* db_slots, uint64_t m, const msc_hist_set* qset,
                 const uint32_t* q_slots, uint64_t n_q, const uint64_t* win_lo, const uint64_t* win_hi, uint32_t top_n, uint64_t* offsets, uint64_t* close_counts,
                 msc_pairs_info* info) {
	if (!ctx || !db || !qset || !offsets || (n_q && !q_slots)) return MSC_ERR_INVALID_ARG;
	if ((cls && cls->ctx != ctx) || (reg && reg->ctx != ctx)) return MSC_ERR_INVALID_ARG;
	if (info) memset(info, 0, sizeof *info);
	ctx->pl_n = 0;          // (the list of the call before is gone whatever happens next)
	ctx->pl_strands = false;
	if (!cls && !reg) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_search_pairs needs a classification or a regression model");
	if (!win_lo != !win_hi) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_search_pairs: win_lo and win_hi are given together or not at all");
	if (m > 0xffffffffull) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_search_pairs: candidate indices are 32-bit");
	memset(offsets, 0, (n_q + 1) * sizeof(uint64_t));
	if (close_counts) memset(close_counts, 0, n_q * sizeof(uint64_t));
	if (n_q == 0 || m == 0) return MSC_OK;
	for (uint64_t i = 0; i < n_q; i++) if (q_slots[i] >= qset->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "query slot out of range");
	int r = validate_pair(ctx, db, qset, q_slots[0], db_slots, m);
	if (r) return r;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	PairsCall c;
	c.ctx = ctx; c.cls = cls; c.reg = reg; c.cands = db; c.cand_slots = db_slots; c.m = m; c.qset = qset; c.q_slots = q_slots; c.n_q = n_q;
	c.top_n = top_n;
	c.windows = win_lo != nullptr;
	if (c.windows) {
		c.win.resize(2 * n_q);
		for (uint64_t q = 0; q < n_q; q++) {
			c.win[n_q + q] = std::min(win_hi[q], m);
			c.win[q] = std::min(win_lo[q], c.win[n_q + q]);
		}
	}
	c.qcount.assign(n_q, 0);
	uint64_t wants[2] = {0, 0};          // the statistics of the classification and of the regression model
	for (int i = 0; i < 2; i++)
		if (const msc_model* md = i ? reg : cls) for (int j = 0; j < md->h.n_singles; j++) wants[i] |= md->h.single_flag[j];
	const uint64_t want = wants[0] | wants[1];
	c.need_emd = (want & MSC_FEAT_EMD) != 0;
	// the matrix-core route: where msc_score_multi would put every block of this call on the product kernel, for both models at once
	// (a divergence statistic leaves it unless msc_set_pairs_div_cells asks for the sums from cells; the 4-bin group statistics always do)
	const uint64_t declines = ctx->pairs_div_cells ? MSC_FEAT_GROUPS : MSC_FEAT_DIV | MSC_FEAT_GROUPS;
	bool matrix = n_q >= 2 && !(want & declines) && kb_route_fits(db, qset, c.need_emd);
	if (matrix) {
		if ((r = ensure_kb(ctx, db)) || (r = ensure_kb(ctx, qset))) return r;
		matrix = db->kb && qset->kb && !db->kb_has_zero && !qset->kb_has_zero;
	}
	plan_blocks(c, 128);
	if (matrix) {
		for (const PairsBlock& b : c.blocks) {          // (a block whose queries' hot list would be too long goes to the older routes there)
			if (block_hot_size(qset, q_slots + b.q0, b.nq) > 64 * (db->L.nbins / 128)) matrix = false;
		}
	}
	if (matrix && c.need_emd) {
		if ((r = ensure_ranks(ctx, db)) || (r = ensure_ranks(ctx, qset))) return r;
		matrix = db->ranks && qset->ranks;
	}
	c.cls_div = matrix && (wants[0] & MSC_FEAT_DIV) != 0;
	c.reg_div = matrix && (wants[1] & MSC_FEAT_DIV) != 0;
	r = matrix ? run_matrix(c) : run_fallback(c);
	if (r) { ctx->pl_n = 0; return r; }
	for (uint64_t q = 0; q < n_q; q++) offsets[q + 1] = offsets[q] + (top_n ? std::min<uint64_t>(c.qcount[q], top_n) : c.qcount[q]);
	if (close_counts) memcpy(close_counts, c.qcount.data(), n_q * sizeof(uint64_t));
	if (offsets[n_q] != ctx->pl_n) { ctx->pl_n = 0; return fail(ctx, MSC_ERR_HIP, "msc_search_pairs: %llu pairs listed, %llu counted", (unsigned long long)ctx->pl_n, (unsigned long long)offsets[n_q]); }
	if (info) {
		info->n_pairs = ctx->pl_n;
		info->route = matrix ? MSC_PAIRS_ROUTE_MATRIX : MSC_PAIRS_ROUTE_FALLBACK;
		info->fp64_pairs = c.fp64;
	}
	return MSC_OK;
}

// the context's scratch set for the reverse complements of n_q queries of qset's shape (a sparse one with an arena of `entries`), emptied
int strand_scratch(msc_ctx* ctx, const msc_hist_set* qset, uint64_t n_q, uint64_t entries) {
	msc_hist_set*& s = ctx->strand_set;
	entries = std::max<uint64_t>(entries, 1);
	if (s && (s->k != qset->k || s->dtype != qset->dtype || s->sparse != qset->sparse || s->capacity < n_q || (s->sparse && s->ent_capacity < entries))) {
		msc_hist_set_destroy(s);
		s = nullptr;
	}
	if (!s) {
		const int r = qset->sparse ? msc_hist_set_create_sparse(ctx, qset->k, qset->dtype, n_q, entries, &s) : msc_hist_set_create(ctx, qset->k, qset->dtype, n_q, &s);
		if (r) {
			s = nullptr;
			const unsigned long long bytes = qset->sparse ? entries * 12ull + n_q * (sizeof(MscSlotScalars) + sizeof(MscSparseHdr)) : n_q * (qset->L.slot_bytes + qset->scalar_stride);
			return fail(ctx, r == MSC_ERR_OOM ? MSC_ERR_OOM : r, "msc_search_pairs_strands: no device memory for the reverse complements of %llu queries (%llu bytes)",
			            (unsigned long long)n_q, bytes);
		}
	}
	if (s->sparse) { if (const int r = msc_hist_set_clear(ctx, s)) return r; }
	s->max_count = s->max_sum = 0;          // (the bounds are the queries' alone: both passes take one route)
	return MSC_OK;
}

}  // namespace

extern "C" int msc_search_pairs_strands(msc_ctx* ctx, const msc_model* cls, const msc_model* reg, const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
                                        const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q, const uint64_t* win_lo, const uint64_t* win_hi, uint64_t* offsets,
                                        msc_pairs_info* info) {
	// the forward pass: every argument check is its
	msc_pairs_info fi{}, ri{};
	int r = search_pairs(ctx, cls, reg, db, db_slots, m, qset, q_slots, n_q, win_lo, win_hi, 0, offsets, nullptr, &fi);
	if (info) memset(info, 0, sizeof *info);
	if (r) return r;
	if (n_q == 0 || m == 0) { ctx->pl_strands = true; return MSC_OK; }
	if (n_q > 0xffffffffull) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_search_pairs_strands: at most 2^32 - 1 queries a call");
	hipStream_t st = ctx->stream;
	std::vector<uint64_t> off_f(offsets, offsets + n_q + 1), off_r(n_q + 1, 0);
	std::swap(ctx->pl_idx, ctx->ps_idx);          // the forward list aside
	std::swap(ctx->pl_sim, ctx->ps_sim);
	ctx->pl_n = 0;
	// the queries' reverse complements, slot i of the scratch set for query i
	uint64_t entries = 0;
	if (qset->sparse) for (uint64_t i = 0; i < n_q; i++) entries += qset->hdr_host[q_slots[i]].nnz;
	if ((r = strand_scratch(ctx, qset, n_q, entries))) return r;
	std::vector<uint32_t> ids(n_q);
	for (uint64_t i = 0; i < n_q; i++) ids[i] = (uint32_t)i;
	if ((r = msc_hist_revcomp_batch(ctx, ctx->strand_set, ids.data(), qset, q_slots, n_q))) return r;
	if ((r = search_pairs(ctx, cls, reg, db, db_slots, m, ctx->strand_set, ids.data(), n_q, win_lo, win_hi, 0, off_r.data(), nullptr, &ri))) return r;
	const uint64_t n_f = off_f[n_q], n_r = off_r[n_q];
	ctx->pl_n = 0;          // (until the merged list stands)
	// the merge
	if ((r = ensure(ctx, ctx->ps_off, 3 * (n_q + 1) * sizeof(uint64_t))) || (r = ensure(ctx, ctx->ps_counts, n_q * sizeof(uint64_t))) ||
	    (r = ensure(ctx, ctx->ps_only, std::max<uint64_t>(n_r, 1) * sizeof(uint32_t))))
		return r;
	uint64_t* d_off_f = (uint64_t*)ctx->ps_off.p;
	uint64_t *d_off_r = d_off_f + n_q + 1, *d_off_m = d_off_r + n_q + 1;
	HIP_TRY(ctx, hipMemcpyAsync(d_off_f, off_f.data(), (n_q + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_off_r, off_r.data(), (n_q + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, msc_launch_pair_strand_count(st, d_off_f, d_off_r, (uint32_t)n_q, (const uint32_t*)ctx->ps_idx.p, (const uint32_t*)ctx->pl_idx.p, (uint32_t*)ctx->ps_only.p,
	                                          (uint64_t*)ctx->ps_counts.p, d_off_m));
	HIP_TRY(ctx, hipMemcpyAsync(offsets, d_off_m, (n_q + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	const uint64_t total = offsets[n_q];
	if (total > n_f + n_r) return fail(ctx, MSC_ERR_HIP, "msc_search_pairs_strands: %llu pairs merged out of %llu + %llu", (unsigned long long)total, (unsigned long long)n_f, (unsigned long long)n_r);
	if ((r = grow_list(ctx, ctx->ps_m_idx, ctx->ps_m_sim, 0, std::max<uint64_t>(total, 1))) || (r = ensure(ctx, ctx->pl_strand, std::max<uint64_t>(total, 1)))) return r;
	HIP_TRY(ctx, msc_launch_pair_strand_write(st, d_off_f, d_off_r, d_off_m, (uint32_t)n_q, (const uint32_t*)ctx->ps_idx.p, (const double*)ctx->ps_sim.p, (const uint32_t*)ctx->pl_idx.p,
	                                          (const double*)ctx->pl_sim.p, (const uint32_t*)ctx->ps_only.p, (uint32_t*)ctx->ps_m_idx.p, (double*)ctx->ps_m_sim.p,
	                                          (uint8_t*)ctx->pl_strand.p));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	std::swap(ctx->pl_idx, ctx->ps_m_idx);          // the merged list is the call's list
	std::swap(ctx->pl_sim, ctx->ps_m_sim);
	ctx->pl_n = total;
	ctx->pl_strands = true;
	if (info) {
		info->n_pairs = total;
		info->fp64_pairs = fi.fp64_pairs + ri.fp64_pairs;
		info->route = fi.route == MSC_PAIRS_ROUTE_MATRIX && ri.route == MSC_PAIRS_ROUTE_MATRIX ? MSC_PAIRS_ROUTE_MATRIX : MSC_PAIRS_ROUTE_FALLBACK;
	}
	return MSC_OK;
}

extern "C" int msc_search_pairs_fetch_strands(msc_ctx* ctx, uint64_t first, uint64_t n, uint8_t* strand) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (!ctx->pl_strands) return fail(ctx, MSC_ERR_UNSUPPORTED, "msc_search_pairs_fetch_strands: the last search was not msc_search_pairs_strands");
	if (first > ctx->pl_n || n > ctx->pl_n - first)
		return fail(ctx, MSC_ERR_INVALID_ARG, "msc_search_pairs_fetch_strands: pairs [%llu, %llu) outside the list of %llu", (unsigned long long)first,
		            (unsigned long long)(first + n), (unsigned long long)ctx->pl_n);
	if (n == 0) return MSC_OK;
	if (!strand) return MSC_ERR_INVALID_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(strand, (const uint8_t*)ctx->pl_strand.p + first, n, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MSC_OK;
}

extern "C" int msc_search_pairs(msc_ctx* ctx, const msc_model* cls, const msc_model* reg, const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
                                const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q, const uint64_t* win_lo, const uint64_t* win_hi, uint64_t* offsets,
                                msc_pairs_info* info) {
	return search_pairs(ctx, cls, reg, db, db_slots, m, qset, q_slots, n_q, win_lo, win_hi, 0, offsets, nullptr, info);
}

extern "C" int msc_search_pairs_top(msc_ctx* ctx, const msc_model* cls, const msc_model* reg, const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
                                    const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q, const uint64_t* win_lo, const uint64_t* win_hi, uint32_t top_n,
                                    uint64_t* offsets, uint64_t* close_counts, msc_pairs_info* info) {
	return search_pairs(ctx, cls, reg, db, db_slots, m, qset, q_slots, n_q, win_lo, win_hi, top_n, offsets, close_counts, info);
}

extern "C" int msc_search_pairs_fetch(msc_ctx* ctx, uint64_t first, uint64_t n, uint32_t* cand_idx, double* sim) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (first > ctx->pl_n || n > ctx->pl_n - first)
		return fail(ctx, MSC_ERR_INVALID_ARG, "msc_search_pairs_fetch: pairs [%llu, %llu) outside the list of %llu", (unsigned long long)first,
		            (unsigned long long)(first + n), (unsigned long long)ctx->pl_n);
	if (n == 0) return MSC_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (cand_idx) HIP_TRY(ctx, hipMemcpyAsync(cand_idx, (const uint32_t*)ctx->pl_idx.p + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	if (sim) HIP_TRY(ctx, hipMemcpyAsync(sim, (const double*)ctx->pl_sim.p + first, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MSC_OK;
}
