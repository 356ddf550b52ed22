// msc_api_pairlist.hip -- msc_score_pair_list (include/meshclust2_hip.h): an explicit list of pairs (a_i, b_i) scored in one pass, the shape of
// the reference's feature table (predict/FeatureSelector.cpp:23-33, predict/Predictor.cpp:876-985). The pairs are grouped by their second slot
// (msc_pair_groups.h); a chunk of the grouped list is one launch of a pair-list kernel -- k_pair_sparse_wl_pairs, k_pair_sparse_mp<.., PAIRS> or
// k_pair_tiles_batch, the kernels of the batched update stage (msc_api_batch.hip) -- and one epilogue, and its rows go back to the caller's
// order on the host. What those kernels do not serve goes query by query through the 1 x M calls. Routes and shared bits: DESIGN.md 4.5b.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "msc_internal.h"

#include "msc_objects.h"
#include "msc_api_private.h"
#include "msc_pair_groups.h"

namespace {

struct PairListOut {
	double *raw, *singles, *combos, *sum, *csum;
	uint8_t* close;
};

// one existing 1 x M call per distinct second slot over that run's first slots, rows scattered back
int pair_list_per_query(msc_ctx* ctx, const msc_model* model, const msc_hist_set* a_set, const uint32_t* a_slots, const msc_hist_set* b_set, const MscPairGroups& g, int order,
                        uint64_t feat_mask, int nf, const PairListOut& o) {
	const int ns = model ? model->h.n_singles : 0, nc = model ? model->h.n_combos : 0;
	std::vector<uint32_t> cands;
	std::vector<double> raw, singles, combos, sum, csum;
	std::vector<uint8_t> close;
	int worst = MSC_OK;
	// a row the reference would throw for holds NaN and the other rows of its run are filled (run_score); the call goes on with the next run and
	// returns the most negative of those statuses, like the epilogue's error word does on the other routes
	auto row_status = [&](int r) -> int { if (r == MSC_ERR_ZERO_LENGTH || r == MSC_ERR_NAN) { worst = std::min(worst, r); return MSC_OK; } return r; };
	for (const MscPairRun& run : g.runs) {
		msc_pair_chunk_a(g, a_slots, run.first, run.first + run.m, cands);
		const uint64_t m = run.m;
		int r;
		if (o.raw) {
			raw.assign((size_t)m * nf, 0.0);
			if ((r = row_status(msc_pair_features_raw(ctx, a_set, cands.data(), m, b_set, run.b_slot, order, feat_mask, raw.data())))) return r;
			msc_pair_scatter(g, run.first, run.first + m, (size_t)nf, raw.data(), o.raw);
		}
		if (model) {
			if (o.singles) singles.assign((size_t)m * ns, 0.0);
			if (o.combos) combos.assign((size_t)m * nc, 0.0);
			sum.assign((size_t)m, 0.0);
			csum.assign((size_t)m, 0.0);
			if ((r = row_status(msc_score(ctx, model, a_set, cands.data(), m, b_set, run.b_slot, order, o.singles ? singles.data() : nullptr, o.combos ? combos.data() : nullptr,
			                              sum.data(), csum.data()))))
				return r;
			if (o.singles) msc_pair_scatter(g, run.first, run.first + m, (size_t)ns, singles.data(), o.singles);
			if (o.combos) msc_pair_scatter(g, run.first, run.first + m, (size_t)nc, combos.data(), o.combos);
			if (o.sum) msc_pair_scatter(g, run.first, run.first + m, 1, sum.data(), o.sum);
			if (o.csum) msc_pair_scatter(g, run.first, run.first + m, 1, csum.data(), o.csum);
			if (o.close) {          // round(classify_sum) > 0, as msc_score_multi's close_out (a NaN row is not close)
				close.resize((size_t)m);
				for (uint64_t i = 0; i < m; i++) close[(size_t)i] = (uint8_t)(std::round(csum[(size_t)i]) > 0 ? 1 : 0);
				msc_pair_scatter(g, run.first, run.first + m, 1, close.data(), o.close);
			}
		}
	}
	// the name of the 1 x M call's kernel, " per query" behind it
	char name[128];
	snprintf(name, sizeof name, "%s", ctx->last_kernel ? ctx->last_kernel : "");
	snprintf(ctx->last_kernel_buf, sizeof ctx->last_kernel_buf, "%s per query", name);
	ctx->last_kernel = ctx->last_kernel_buf;
	ctx->last_query_tile = 1;
	if (worst == MSC_ERR_ZERO_LENGTH) return fail(ctx, worst, "length_difference: a point has length 0 (the reference throws 123, predict/Feature.cpp:878-886)");
	if (worst == MSC_ERR_NAN) return fail(ctx, worst, "normalisation produced NaN (the reference throws, predict/Feature.cpp:143-146)");
	return MSC_OK;
}

}  // namespace

extern "C" int msc_score_pair_list(msc_ctx* ctx, const msc_model* model, const msc_hist_set* a_set, const uint32_t* a_slots, const msc_hist_set* b_set,
                                   const uint32_t* b_slots, uint64_t n, int order, uint64_t feat_mask, double* raw_out, double* singles_out, double* combos_out,
                                   double* sum_out, double* csum_out, uint8_t* close_out) {
	if (!ctx || !a_set || !b_set || a_set->ctx != ctx || b_set->ctx != ctx || (model && model->ctx != ctx)) return MSC_ERR_INVALID_ARG;
	// (the checks of the 1 x M calls, validate_pair: the fallback below is made of those calls, so what they refuse is refused here)
	if (a_set->k != b_set->k || a_set->dtype != b_set->dtype || a_set->sparse != b_set->sparse)
		return fail(ctx, MSC_ERR_INVALID_ARG, "the two sets differ in k, dtype or layout");
	if (model && model->k != a_set->k) return fail(ctx, MSC_ERR_INVALID_ARG, "the model is of k = %d, the sets of k = %d", model->k, a_set->k);
	if (order != MSC_ORDER_CAND_FIRST && order != MSC_ORDER_QUERY_FIRST) return fail(ctx, MSC_ERR_INVALID_ARG, "order is MSC_ORDER_CAND_FIRST or MSC_ORDER_QUERY_FIRST");
	if (n == 0) return MSC_OK;
	const bool model_out = singles_out || combos_out || sum_out || csum_out || close_out;
	if (!raw_out && !model_out) return fail(ctx, MSC_ERR_INVALID_ARG, "every output pointer is NULL");
	if (model_out && !model) return fail(ctx, MSC_ERR_INVALID_ARG, "singles / combos / sum / csum / close need a model");
	if (!model_out) model = nullptr;
	if (raw_out && (feat_mask == 0 || (feat_mask & ~kSupportedFeats)))
		return fail(ctx, MSC_ERR_UNSUPPORTED, "feat_mask 0x%llx holds statistics outside the GPU path (supported 0x%llx)", (unsigned long long)feat_mask,
		            (unsigned long long)kSupportedFeats);
	if (!raw_out) feat_mask = 0;
	if (n > 0xfffffff0ull) return fail(ctx, MSC_ERR_INVALID_ARG, "too many pairs in one call");
	if (a_slots) { for (uint64_t i = 0; i < n; i++) if (a_slots[i] >= a_set->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "first slot %u out of range", a_slots[i]); }
	else if (n > a_set->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "n exceeds the first set's capacity");
	if (b_slots) { for (uint64_t i = 0; i < n; i++) if (b_slots[i] >= b_set->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "second slot %u out of range", b_slots[i]); }
	else if (n > b_set->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "n exceeds the second set's capacity");
	HIP_TRY(ctx, hipSetDevice(ctx->device));

	const MscLayout& L = a_set->L;
	const int nf = __builtin_popcountll(feat_mask);
	const int ns = model ? model->h.n_singles : 0, ncb = model ? model->h.n_combos : 0;
	uint64_t want = feat_mask;
	for (int i = 0; i < ns; i++) want |= model->h.single_flag[i];
	const bool want_div = (want & MSC_FEAT_DIV) != 0;
	const PairListOut out{raw_out, singles_out, combos_out, sum_out, csum_out, close_out};
	const MscPairGroups g = msc_pair_group(b_slots, n);
	ctx->tiles_ms_accum = 0.f;
	ctx->tiles_launches = 0;
	ctx->have_timing = false;

	// ---- the route
	const bool sp = a_set->sparse;
	int r;
	bool per_query = needs_wide(a_set, b_set) || (want & MSC_FEAT_GROUPS) != 0 || (sp && std::max(a_set->max_count, b_set->max_count) >= 65536);
	const msc_hist_set *c_sp = nullptr, *q_sp = nullptr;          // the lists a pass merges: the sets themselves, or the sparse mirrors of dense sets
	if (!per_query) {
		if (sp) { c_sp = a_set; q_sp = b_set; }
		else {
			if (mirror_pass_allowed(ctx, L)) {
				if ((r = ensure_sparse_mirror(ctx, a_set, &c_sp)) || (r = ensure_sparse_mirror(ctx, b_set, &q_sp))) return r;
				if (!c_sp || !q_sp) c_sp = q_sp = nullptr;
			}
		}
		if (want_div) {
			// the two sums come from the pair-list form of the chunked merge kernel or not from here at all: a pair keeps its one evaluation order
			bool ok = false;
			if (!c_sp) per_query = true;
			else if ((r = batch_div_lists(ctx, a_set, b_set, g.runs[0].b_slot, &c_sp, &q_sp, &ok))) return r;
			else per_query = !ok;
		}
	}
	if (per_query) return pair_list_per_query(ctx, model, a_set, a_slots, b_set, g, order, feat_mask, nf, out);

	const bool lists = c_sp != nullptr;
	const bool wl = lists && !want_div && msc_sparse_wl_pairs_fits(c_sp->max_nnz, q_sp->max_nnz);
	ctx->last_kernel = !lists ? "k_pair_tiles_batch" : wl ? "k_pair_sparse_wl_pairs" : "k_pair_sparse_mp";
	ctx->last_query_tile = 1;
	const uint32_t PS = lists ? 1 : L.S;          // partial records per pair
	ctx->last_partial_stride = PS;
	// chunks of the grouped list, by the scratch budgets of the batched update stage (partial records; a 4 KiB table of divergence terms per
	// pair) and 512 MiB of result rows
	const uint64_t row_bytes = (uint64_t)nf * 8 + (singles_out ? (uint64_t)ns * 8 : 0) + (combos_out ? (uint64_t)ncb * 8 : 0) + 24;
	uint64_t max_pairs = std::max<uint64_t>(1, (2048ull << 20) / ((uint64_t)PS * sizeof(MscPartial)));
	if (want_div) max_pairs = std::min<uint64_t>(max_pairs, (1024ull << 20) / 4096);
	max_pairs = std::min<uint64_t>(max_pairs, std::max<uint64_t>(1024, (512ull << 20) / row_bytes));
	const std::vector<uint64_t> cuts = msc_pair_chunks(n, max_pairs);

	std::vector<MscPairRun> runs;
	std::vector<MscBatchSeg> segs;
	std::vector<uint32_t> pair_seg, cands;
	std::vector<double> h_raw, h_singles, h_combos, h_sum, h_csum;
	std::vector<uint8_t> h_close;
	int32_t first_err = 0;
	if ((r = ensure(ctx, ctx->err_word, sizeof(int32_t)))) return r;
	HIP_TRY(ctx, hipMemsetAsync(ctx->err_word.p, 0, sizeof(int32_t), ctx->stream));
	for (size_t ch = 0; ch + 1 < cuts.size(); ch++) {
		const uint64_t p0 = cuts[ch], p1 = cuts[ch + 1], P = p1 - p0;
		uint64_t max_m = 0;
		msc_pair_chunk_runs(g, p0, p1, runs, pair_seg, &max_m);
		msc_pair_chunk_a(g, a_slots, p0, p1, cands);
		segs.resize(runs.size());
		for (size_t s = 0; s < runs.size(); s++) {
			MscBatchSeg& sg = segs[s];
			sg.q_slot = runs[s].b_slot;
			sg.first = (uint32_t)runs[s].first;
			sg.m = (uint32_t)runs[s].m;
			sg.pad_ = 0;
			// no length window. batch_div_pass launches its kernel with use_window = 1 (the batched update stage, whose helper it is, always
			// has one), so the divergence route is right only because every segment carries the window that lets every length through
			sg.min_len = 0;
			sg.max_len = ~0ull;
		}
		if ((r = ensure(ctx, ctx->segs, segs.size() * sizeof(MscBatchSeg))) || (r = ensure(ctx, ctx->pair_seg, P * sizeof(uint32_t))) ||
		    (r = ensure(ctx, ctx->slots, P * sizeof(uint32_t))) || (r = ensure(ctx, ctx->partials, P * PS * sizeof(MscPartial))))
			return r;
		if (raw_out && (r = ensure(ctx, ctx->raw, P * nf * sizeof(double)))) return r;
		if (singles_out && (r = ensure(ctx, ctx->singles, P * ns * sizeof(double)))) return r;
		if (combos_out && (r = ensure(ctx, ctx->combos, P * ncb * sizeof(double)))) return r;
		if (sum_out && (r = ensure(ctx, ctx->soa_sum, P * sizeof(double)))) return r;
		if (csum_out && (r = ensure(ctx, ctx->soa_csum, P * sizeof(double)))) return r;
		if (close_out && (r = ensure(ctx, ctx->soa_close, P))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->segs.p, segs.data(), segs.size() * sizeof(MscBatchSeg), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->pair_seg.p, pair_seg.data(), P * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->slots.p, cands.data(), P * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		if (ctx->timing && ch == 0) HIP_TRY(ctx, hipEventRecord(ctx->ev_all0, ctx->stream));
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles0, ctx->stream));
		uint32_t dvn = 1;          // {jd, js} records per pair
		if (want_div) {
			// (the divergence form leaves the pair's integer record as well: one launch serves both)
			if ((r = batch_div_pass(ctx, a_set, b_set, c_sp, q_sp, P, order, (MscPartial*)ctx->partials.p, &dvn))) return r;
		} else if (wl)
			HIP_TRY(ctx, msc_launch_pair_sparse_wl_pairs(ctx->stream, c_sp->ent, c_sp->cum, c_sp->hdr, (const uint32_t*)ctx->slots.p, (uint32_t)P, q_sp->ent, q_sp->cum, q_sp->hdr,
			                                             (const MscBatchSeg*)ctx->segs.p, (const uint32_t*)ctx->pair_seg.p, c_sp->max_nnz, q_sp->max_nnz, L.nbins,
			                                             (MscPartial*)ctx->partials.p, ctx->num_cus));
		else if (lists)
			HIP_TRY(ctx, msc_launch_pair_sparse_mp_pairs(ctx->stream, c_sp->ent, c_sp->cum, c_sp->hdr, a_set->scalars, a_set->scalar_stride, (const uint32_t*)ctx->slots.p, (uint32_t)P,
			                                             q_sp->ent, q_sp->cum, q_sp->hdr, L.nbins, 0, (const MscBatchSeg*)ctx->segs.p, (const uint32_t*)ctx->pair_seg.p,
			                                             (MscPartial*)ctx->partials.p, order, ctx->num_cus));
		else
			HIP_TRY(ctx, msc_launch_pair_tiles_batch(ctx->stream, L, a_set->dtype, a_set->bins, a_set->scalars, (const uint32_t*)ctx->slots.p, (const MscBatchSeg*)ctx->segs.p,
			                                         (uint32_t)segs.size(), (uint32_t)max_m, b_set->bins, b_set->L.slot_bytes, b_set->scalars, b_set->scalar_stride, 0,
			                                         (MscPartial*)ctx->partials.p, order));
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles1, ctx->stream));
		MscEpilogueArgs ea;
		memset(&ea, 0, sizeof ea);
		ea.partials = (const MscPartial*)ctx->partials.p;
		if (want_div) { ea.div_direct = (const double*)ctx->div_partials.p; ea.div_direct_n = dvn; ea.div_base = L.nbins; }
		ea.S = PS;
		ea.sparse_base = lists ? L.nbins : 0;
		ea.m = (uint32_t)P;
		ea.cand_scalars = a_set->scalars;          // (the scalar records are the sets' own: a mirror has none)
		ea.cand_scalar_stride = a_set->scalar_stride;
		ea.cand_slots = (const uint32_t*)ctx->slots.p;
		ea.q_scalars = b_set->scalars;
		ea.qset_scalars = b_set->scalars;
		ea.q_scalar_stride = b_set->scalar_stride;
		ea.nbins = L.nbins;
		ea.dtype = a_set->dtype;
		ea.order = order;
		ea.use_window = 0;
		ea.feat_mask = feat_mask;
		ea.raw_out = raw_out ? (double*)ctx->raw.p : nullptr;
		ea.model = model ? model->d : nullptr;
		ea.singles_out = singles_out ? (double*)ctx->singles.p : nullptr;
		ea.combos_out = combos_out ? (double*)ctx->combos.p : nullptr;
		ea.sum_soa = sum_out ? (double*)ctx->soa_sum.p : nullptr;
		ea.csum_soa = csum_out ? (double*)ctx->soa_csum.p : nullptr;
		ea.close_soa = close_out ? (uint8_t*)ctx->soa_close.p : nullptr;
		ea.error_word = (int32_t*)ctx->err_word.p;
		ea.segs = (const MscBatchSeg*)ctx->segs.p;
		ea.pair_seg = (const uint32_t*)ctx->pair_seg.p;
		if (raw_out && model) {
			// two evaluations, as the per-pair calls are two: a row's model outputs must not turn NaN over a statistic only feat_mask asked for
			MscEpilogueArgs er = ea;
			er.model = nullptr;
			er.singles_out = er.combos_out = er.sum_soa = er.csum_soa = nullptr;
			er.close_soa = nullptr;
			HIP_TRY(ctx, msc_launch_epilogue(ctx->stream, er));
			ea.raw_out = nullptr;
			ea.feat_mask = 0;
		}
		HIP_TRY(ctx, msc_launch_epilogue(ctx->stream, ea));
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all1, ctx->stream));
		// rows of the chunk to the host, then to the caller's order
		if (raw_out) { h_raw.resize((size_t)P * nf); HIP_TRY(ctx, hipMemcpyAsync(h_raw.data(), ctx->raw.p, h_raw.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream)); }
		if (singles_out) { h_singles.resize((size_t)P * ns); HIP_TRY(ctx, hipMemcpyAsync(h_singles.data(), ctx->singles.p, h_singles.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream)); }
		if (combos_out) { h_combos.resize((size_t)P * ncb); HIP_TRY(ctx, hipMemcpyAsync(h_combos.data(), ctx->combos.p, h_combos.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream)); }
		if (sum_out) { h_sum.resize((size_t)P); HIP_TRY(ctx, hipMemcpyAsync(h_sum.data(), ctx->soa_sum.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, ctx->stream)); }
		if (csum_out) { h_csum.resize((size_t)P); HIP_TRY(ctx, hipMemcpyAsync(h_csum.data(), ctx->soa_csum.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, ctx->stream)); }
		if (close_out) { h_close.resize((size_t)P); HIP_TRY(ctx, hipMemcpyAsync(h_close.data(), ctx->soa_close.p, (size_t)P, hipMemcpyDeviceToHost, ctx->stream)); }
		HIP_TRY(ctx, hipMemcpyAsync(&first_err, ctx->err_word.p, sizeof first_err, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		float t = 0;
		if (ctx->timing && hipEventElapsedTime(&t, ctx->ev_tiles0, ctx->ev_tiles1) == hipSuccess) { ctx->tiles_ms_accum += t; ctx->tiles_launches++; ctx->have_timing = true; }
		if (raw_out) msc_pair_scatter(g, p0, p1, (size_t)nf, h_raw.data(), raw_out);
		if (singles_out) msc_pair_scatter(g, p0, p1, (size_t)ns, h_singles.data(), singles_out);
		if (combos_out) msc_pair_scatter(g, p0, p1, (size_t)ncb, h_combos.data(), combos_out);
		if (sum_out) msc_pair_scatter(g, p0, p1, 1, h_sum.data(), sum_out);
		if (csum_out) msc_pair_scatter(g, p0, p1, 1, h_csum.data(), csum_out);
		if (close_out) msc_pair_scatter(g, p0, p1, 1, h_close.data(), close_out);
	}
	if (first_err == MSC_ERR_ZERO_LENGTH) return fail(ctx, first_err, "length_difference: a point has length 0 (the reference throws 123, predict/Feature.cpp:878-886)");
	if (first_err == MSC_ERR_NAN) return fail(ctx, first_err, "normalisation produced NaN (the reference throws, predict/Feature.cpp:143-146)");
	if (first_err < 0) return fail(ctx, first_err, "feature evaluation failed with status %d", first_err);
	return MSC_OK;
}
