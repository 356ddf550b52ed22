// msc_api_score.hip -- the scoring driver behind the C ABI's 1 x M calls (include/meshclust2_hip.h): run_score -- which kernel takes a pass, its
// scratch, the epilogue and the reduction -- and msc_pair_features_raw / msc_score / msc_get_close / msc_filter / msc_merge / msc_search /
// msc_mean_nearest (Trainer::get_close / filter / merge / closest, cluster/Trainer.cpp:23-157). Split from msc_api.hip in r05.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "msc_internal.h"

#include "msc_objects.h"
#include "msc_api_private.h"

// ================================================================================================ scoring driver


// integer range of the fast streaming kernels (pair_features.hip header); outside it the 64-bit kernel runs
bool needs_wide(const msc_hist_set* a, const msc_hist_set* b) {
	const uint64_t mc = std::max(a->max_count, b->max_count), ms = std::max(a->max_sum, b->max_sum);
	// a lane adds the |prefix difference| of its R bins of a tile in 32 bits; a prefix difference is at most the larger excess
	// (k-mer) total, so R * excess must stay below 2^32 (only sequences of >= 2^26 k-mers can break it)
	const uint64_t excess = ms > a->L.nbins ? ms - a->L.nbins : 0;
	return mc > kNarrowMaxCount || ms > kNarrowMaxSum || (uint64_t)a->L.R * excess >= (1ull << 32);
}

int validate_pair(msc_ctx* ctx, const msc_hist_set* cands, const msc_hist_set* qset, uint64_t q_slot, const uint32_t* slots, uint64_t m) {
	if (!ctx || !cands || !qset || cands->ctx != ctx || qset->ctx != ctx) return MSC_ERR_INVALID_ARG;
	if (cands->k != qset->k || cands->dtype != qset->dtype || cands->sparse != qset->sparse)
		return fail(ctx, MSC_ERR_INVALID_ARG, "query and candidate sets differ in k, dtype or layout");
	if (q_slot >= qset->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "query slot out of range");
	if (m > 0xfffffff0ull) return fail(ctx, MSC_ERR_INVALID_ARG, "too many candidates in one call");
	if (slots) { for (uint64_t i = 0; i < m; i++) if (slots[i] >= cands->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "candidate slot %u out of range", slots[i]); }
	else if (m > cands->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "m exceeds capacity");
	return MSC_OK;
}

// Which merge kernel scores a query list against candidate lists -- one rule for sparse sets and for the sparse mirrors of dense
// sets, so a pair gets the same kernel (hence the same evaluation order of the FP64 divergence sums) in every route:
//   SPK_LDS     whole lists in LDS (MSC_SPARSE_LDS=1; kept for comparison), 32-bit range, one record per candidate
//   SPK_MP      merge-path chunks, 32-bit range (counts < 2^16, sums < 2^31), one record per candidate
//   SPK_GENERIC lane per index sub-range straight from global memory, 64-bit running values, 16 records per candidate
SparseKernel pick_sparse_kernel(const msc_hist_set* c_sp, const msc_hist_set* q_sp, uint64_t q_slot, uint64_t max_count, bool wide) {
	static const bool want_lds = getenv("MSC_SPARSE_LDS") != nullptr;
	static const bool no_mp = getenv("MSC_SPARSE_NO_MP") != nullptr;
	const uint64_t q_nnz = q_sp->hdr_host[q_slot].nnz;
	if (want_lds && !wide && max_count < 65536 && c_sp->L.nbins >= 64 && ((size_t)(q_nnz + 128) + 4ull * (c_sp->max_nnz + 128)) * 8 <= 96 * 1024) return SPK_LDS;
	if (!no_mp && !wide && max_count < 65536 && q_nnz + c_sp->max_nnz <= msc_sparse_mp_max_entries()) return SPK_MP;
	return SPK_GENERIC;
}
uint32_t sparse_records(SparseKernel k, uint32_t mp_parts) { return k == SPK_GENERIC ? MSC_SPARSE_SUB : k == SPK_MP ? mp_parts : 1; }
// {jd, js} records per pair: the merge-path kernel leaves one per granule of the merged order (lists of up to `entries` together)
uint32_t div_records(SparseKernel k, uint64_t entries) { return k == SPK_GENERIC ? MSC_SPARSE_SUB : k == SPK_MP ? msc_sparse_mp_div_records(entries) : 1; }
const char* sparse_kernel_name(SparseKernel k) { return k == SPK_LDS ? "k_pair_sparse_lds" : k == SPK_MP ? "k_pair_sparse_mp" : "k_pair_sparse"; }

// candidates [off, off + mc) (or the device slot list d_slots) of the sparse set / mirror c_sp against slot q_slot of q_sp; the
// scalar records are those of the sets the lists belong to (a mirror has none of its own)
hipError_t launch_sparse_pass(msc_ctx* ctx, SparseKernel k, const msc_hist_set* c_sp, const uint8_t* c_scalars, uint64_t c_stride, const uint32_t* d_slots,
                              uint64_t off, uint32_t mc, const msc_hist_set* q_sp, uint64_t q_slot, const uint8_t* q_scal, uint64_t nbins, int use_window,
                              uint64_t min_len, uint64_t max_len, MscPartial* partials, void* div_tables, void* div_partials, int order, uint32_t parts,
                              uint32_t div_stride) {
	const MscSparseHdr* c_hdr = c_sp->hdr + (d_slots ? 0 : off);
	const uint8_t* c_scal = c_scalars + (d_slots ? 0 : off * c_stride);
	const uint32_t q_nnz = q_sp->hdr_host[q_slot].nnz;
	if (k == SPK_LDS)
		return msc_launch_pair_sparse_lds(ctx->stream, c_sp->ent, c_sp->cum, c_hdr, c_scal, c_stride, d_slots, mc, q_sp->ent, q_sp->cum, q_sp->hdr + q_slot, q_scal, nbins,
		                                  q_nnz, c_sp->max_nnz, use_window, min_len, max_len, partials, div_tables, div_partials, order, ctx->num_cus);
	if (k == SPK_MP)
		return msc_launch_pair_sparse_mp(ctx->stream, c_sp->ent, c_sp->cum, c_hdr, c_scal, c_stride, d_slots, mc, q_sp->ent, q_sp->cum, q_sp->hdr + q_slot, q_scal, nbins,
		                                 use_window, min_len, max_len, partials, div_tables, div_partials, order, ctx->num_cus,
		                                 (uint32_t)std::min<uint64_t>(0x7fffffffull, (uint64_t)q_nnz + c_sp->max_nnz), parts, q_nnz, c_sp->max_nnz, div_stride);
	return msc_launch_pair_sparse(ctx->stream, c_sp->ent, c_sp->cum, c_hdr, c_scal, c_stride, d_slots, mc, q_sp->ent, q_sp->cum, q_sp->hdr + q_slot, q_scal, nbins,
	                              use_window, min_len, max_len, partials, div_tables, div_partials, order);
}

// The two list caches of a set -- its rank lists and its repeated-bin lists -- are built alike: the slots' sizes and offsets, the total read
// back, the entry array grown with 1/8 slack, the fill. *no_memory: an allocation failed (nothing reported: what follows is the caller's policy)
template <class E, class Sizes, class Fill>
static int build_slot_lists(msc_ctx* ctx, uint64_t capacity, uint64_t*& off, uint32_t*& n, E*& ent, uint64_t& entries, bool* no_memory, Sizes sizes, Fill fill) {
	*no_memory = true;
	if (!off && (hipMalloc((void**)&off, (capacity + 1) * sizeof(uint64_t)) != hipSuccess || hipMalloc((void**)&n, capacity * sizeof(uint32_t)) != hipSuccess)) return MSC_ERR_OOM;
	*no_memory = false;
	HIP_TRY(ctx, sizes());
	uint64_t total = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&total, off + capacity, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (total + 4 > entries) {
		if (ent) (void)hipFree(ent);
		ent = nullptr;
		entries = total + total / 8 + 1024;
		if (hipMalloc((void**)&ent, entries * sizeof(E)) != hipSuccess) { entries = 0; *no_memory = true; return MSC_ERR_OOM; }
	}
	HIP_TRY(ctx, fill());
	return MSC_OK;
}

// The rank lists of the sparse set (or sparse mirror) `s`, for the 1 x M pass of msc_ranks_pass.hip: true when they are current. Built only
// once the same state of the set has been asked for three times (msc_objects.h).
bool rank_lists_ready(msc_ctx* ctx, const msc_hist_set* s, int* err, bool eager) {
	*err = MSC_OK;
	if (!s->sparse || s->rkl_unavailable) return false;
	if (s->rkl && s->rkl_epoch == s->list_epoch) return true;
	if (s->rkl_seen_epoch != s->list_epoch) { s->rkl_seen_epoch = s->list_epoch; s->rkl_seen = 0; }
	// (MSC_RANKS_1XM_AFTER=n: build at the n-th request instead of the third; read on every call so that a test can switch it)
	const char* after_env = getenv("MSC_RANKS_1XM_AFTER");
	const uint32_t after = after_env && atoi(after_env) > 0 ? (uint32_t)atoi(after_env) : 3u;
	// eager: the step-serial loop's own call (msc_get_close_window over a sealed store) builds at its FIRST pass -- which kernel scores a
	// candidate must not depend on how many passes its rank has seen (a rank whose window was empty for a step would otherwise switch a
	// step later than the others, and two identical sequences on two ranks would differ in the last bit of a divergence sum)
	if (!eager && ++s->rkl_seen < after) return false;
	bool no_memory = false;
	*err = build_slot_lists(
	    ctx, s->capacity, s->rkl_off, s->rkl_n, s->rkl, s->rkl_entries, &no_memory,
	    [&] { return msc_launch_rank_lists_sizes(ctx->stream, s->hdr, s->cum, s->capacity, s->rkl_n, s->rkl_off); },
	    [&] { return msc_launch_rank_lists_fill(ctx->stream, s->ent, s->cum, s->hdr, s->capacity, s->rkl_n, s->rkl_off, s->L.nbins, s->rkl); });
	if (no_memory) {
		// (no memory for the lists: the merge kernels stay -- except in the step-serial loop's own call, where it is an error: which kernel scores
		// a pass there must not depend on what one rank's allocator had left)
		(void)hipGetLastError();
		*err = eager ? fail(ctx, MSC_ERR_OOM, "rank lists: out of device memory") : MSC_OK;
		if (!eager) s->rkl_unavailable = true;
		return false;
	}
	if (*err) return false;
	s->rkl_off_host.resize(s->capacity + 1);
	if (hipMemcpyAsync(s->rkl_off_host.data(), s->rkl_off, (s->capacity + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
		*err = fail(ctx, MSC_ERR_HIP, "rank lists: offsets read-back failed");
		return false;
	}
	s->rkl_epoch = s->list_epoch;
	return true;
}

// ... and its repeated-bin lists, which the long-list pass (k_pair_ranks_items) reads beside them: built at the first such pass of an epoch;
// no memory for them is always an error
static int rank_multi_ready(msc_ctx* ctx, const msc_hist_set* s) {
	if (s->rkm && s->rkm_epoch == s->list_epoch) return MSC_OK;
	bool no_memory = false;
	const int r = build_slot_lists(
	    ctx, s->capacity, s->rkm_off, s->rkm_n, s->rkm, s->rkm_entries, &no_memory,
	    [&] { return msc_launch_rank_multi_sizes(ctx->stream, s->ent, s->hdr, s->capacity, s->rkm_n, s->rkm_off); },
	    [&] { return msc_launch_rank_multi_fill(ctx->stream, s->ent, s->hdr, s->capacity, s->rkm_off, s->rkm); });
	if (no_memory) {
		(void)hipGetLastError();
		return fail(ctx, MSC_ERR_OOM, "repeated-bin lists: out of device memory");
	}
	if (r) return r;
	s->rkm_epoch = s->list_epoch;
	return MSC_OK;
}

// ================================================================================================ the route of a 1 x M call

bool mirror_pass_allowed(const msc_ctx* ctx, const MscLayout& L) {
	static const bool no_mirror_env = getenv("MSC_NO_SPARSE_MIRROR") != nullptr;
	return !no_mirror_env && ctx->mirror_pass && L.nbins == L.padded_bins;
}

int pair_status(msc_ctx* ctx, int first_err) {
	if (first_err == MSC_ERR_ZERO_LENGTH) return fail(ctx, first_err, "length_difference: a point has length 0 (the reference throws 123, predict/Feature.cpp:878-886)");
	if (first_err == MSC_ERR_NAN) return fail(ctx, first_err, "normalisation produced NaN (the reference throws, predict/Feature.cpp:143-146)");
	if (first_err < 0) return fail(ctx, first_err, "feature evaluation failed with status %d", first_err);
	return MSC_OK;
}

namespace {

enum PassKind { PASS_TILES, PASS_TILES_WIDE, PASS_MERGE, PASS_RANKS_1XM, PASS_RANKS_ITEMS };          // which kernel streams the candidates
// where the two FP64 divergence sums come from: the table form inside k_pair_tiles / the direct form inside the wide kernel, a merge pass over
// the mirror's lists beside the streaming kernel, the merge pass itself, the cells the items kernel counts
enum DivForm { DIV_NONE, DIV_INLINE, DIV_MIRROR, DIV_LISTS, DIV_RANKS };
enum GroupForm { GRP_NONE, GRP_DENSE, GRP_LISTS };          // sim_mm / rre_k_r: the dense group kernels, or from the lists

// what pick_score_route decides for one call; the stages below read it and decide nothing
struct ScoreRoute {
	PassKind pass = PASS_TILES;
	DivForm div = DIV_NONE;          // (DIV_MIRROR and up: c_sp exists and the sums reach the epilogue per {jd, js} record)
	GroupForm grp = GRP_NONE;
	const msc_hist_set *c_sp = nullptr, *q_sp = nullptr;          // the lists the pass or its side passes read: the sets themselves or their sparse mirrors
	SparseKernel spk = SPK_GENERIC;                                // the merge kernel of the pass / of the mirror side pass
	uint32_t mp_parts = 1;                                         // waves that share a candidate of the merge-path kernel
	uint32_t PS = 0, SPN = 0, DVN = 0;                             // records per candidate: partials of the pass, of a merge pass, {jd, js}
	uint32_t rank_rounds = 0;                                      // items pass: rounds of 1 024 entries that cover its longest list
	uint64_t q_kmers = 0, chunk = 0;                               // bound on the k-mers of any histogram of the query's set; candidates per chunk
	int nf = 0, ns = 0, nc = 0;                                    // raw statistics, singles, combos per candidate
	bool need_po = false, fused = false;                           // the per-pair records go home; epilogue, first reduce stage and close pass in one kernel
	const char* kernel = "";                                       // msc_last_kernel_info's name of the pass
	bool lists() const { return pass >= PASS_MERGE; }              // the pass reads two lists, no bins
	bool ranks() const { return pass >= PASS_RANKS_1XM; }
};

// one chunk of the candidates
struct ScoreChunk {
	uint64_t off = 0;
	uint32_t mc = 0;
	const uint32_t* d_slots = nullptr;
	const uint8_t *c_bins = nullptr, *c_scal = nullptr, *q_bins = nullptr, *q_scal = nullptr;
};

// what the stages of a chunk hand on, and what the call keeps of its chunks
struct ScoreHome {
	std::vector<MscPairOut> po;
	int first_err = 0;
	bool fold_on_host = false;          // the fused kernel's parts sit in page-locked memory: the host folds them behind the wait
	uint32_t n_parts = 0;
};

// May the pass run over RANK lists, and which of the two rank kernels takes it? Sets pass, rank_rounds and the kernel's name.
int pick_rank_pass(msc_ctx* ctx, const ScoreRequest& rq, bool need_div, ScoreRoute* rt) {
	const MscLayout& L = rq.cands->L;
	const msc_hist_set *c_sp = rt->c_sp, *q_sp = rt->q_sp;
	int r;
	// r04: up to k = 9 the integer statistics of a list pass come from RANK lists -- no merge (msc_ranks_pass.hip): the query's histogram as
	// two bits per bin in LDS, the candidates' k-mers streamed at 4 bytes each. Same records as the merge kernels, bit for bit.
	const bool no_rank_pass = getenv("MSC_NO_RANKS_1XM") != nullptr;          // (read on every call: tests compare both routes in one process)
	// (the divergence statistics too: bins counted per cell of (candidate's count, query's count) by k_pair_ranks_items, evaluated per
	// candidate in one fixed order by k_rank_items_finish -- msc_ranks_pass.hip; MSC_NO_RANKS_DIV keeps such passes on the merge kernel)
	const bool no_rank_div = getenv("MSC_NO_RANKS_DIV") != nullptr;
	// ... and only in the step-serial loop's own call (msc_get_close_window: rq.close_list) unless MSC_RANKS_DIV asks for it everywhere: the
	// two FP64 sums of the rank form add the same terms in another order than the merge kernel's (they agree to ~1e-15 relative), and every
	// OTHER route -- 1 x M by slot list, Q x M, the batched update stage, dense or sparse -- keeps returning bit-identical values for a pair
	// (test_divergence_statistics_are_the_same_in_every_route). Within a window pass all candidates come from one kernel, so
	// ties among them are decided as before.
	const bool rank_div_wanted = rq.close_list.pos != nullptr || getenv("MSC_RANKS_DIV") != nullptr;
	// Long lists (more than 8 192 k-mers on either side) go through k_pair_ranks_items: the unit of work is a round of 1 024 entries of a
	// candidate, so a window of a few thousand long candidates still fills the chip (MSC_NO_RANKS_ITEMS: such passes stay on the merge kernel
	// when they carry divergence statistics, on k_pair_ranks_1xm otherwise).
	const uint64_t c_kmers = c_sp->max_sum >= L.nbins ? c_sp->max_sum - L.nbins : ~0ull;          // bound on the k-mers of any candidate
	// (which of the two rank kernels takes a pass is decided by the QUERY alone -- its stored bins, the same number on every rank of a sharded
	// run and in a one-rank run -- never by a bound of the set or shard at hand: the two kernels add the divergence terms in different orders,
	// and two identical sequences scored for one query must not come out one bit apart because they sit on different ranks)
	// r05: a pass that carries the divergence statistics takes the items kernel whatever the query's length (cfg5's shape, the 3 461 passes
	// of short queries among 14 719: 22 us against 137 + 31 + 9 of k_pair_ranks_1xm's divergence form, its finish and the query's two
	// preparation kernels); without them a short query's pass stays with k_pair_ranks_1xm (1 kb +- 100, 13 300 candidates per pass: 31 us
	// against 35 + 10 + 6.5). (MSC_RANKS_ITEMS_FROM=n: the bound for both.)
	static const int items_from = [] { const char* e = getenv("MSC_RANKS_ITEMS_FROM"); return e ? atoi(e) : -1; }();
	const bool long_lists = q_sp->hdr_host[rq.q_slot].nnz > (uint32_t)(items_from >= 0 ? items_from : need_div ? 0 : 2000);
	// Rounds of 1 024 entries that cover the longest list THIS PASS can meet: a candidate the length window drops takes no
	// round, so inside a window no list is longer than max_len k-mers (nor the query's own); only without a window does the set's bound
	// count. One 50 Mb scaffold among short sequences used to size -- and clear, every step -- the accumulators of every pass for 50 000
	// rounds per candidate. And a pass whose scratch would still pass 2 GiB stays with the merge kernels instead of failing with OOM.
	uint64_t pass_kmers = std::max(rt->q_kmers, c_kmers);
	if (rq.use_window && long_lists) {
		uint64_t q_len = 0;
		if ((r = slot_length(ctx, rq.qset, rq.q_slot, &q_len))) return r;
		pass_kmers = std::min(pass_kmers, std::max(rq.max_len, q_len));
	}
	const uint64_t pass_rounds = (pass_kmers + msc_ranks_items_round() - 1) / msc_ranks_items_round();
	const bool items_ok = getenv("MSC_NO_RANKS_ITEMS") == nullptr && c_kmers < (1ull << 26) && pass_rounds < (1ull << 26) && rq.m * (64 + pass_rounds * 3 * 280) <= (2048ull << 20);
	const bool div_fits = !need_div || (!no_rank_div && rank_div_wanted && long_lists && items_ok);          // (only the items kernel carries the divergence statistics)
	if (!rt->lists() || !div_fits || rq.only_tiles || rt->spk != SPK_MP || no_rank_pass || rt->q_kmers > msc_ranks_pass_query_cap() || msc_ranks_pass_lds(L.nbins, rt->q_kmers) == 0)
		return MSC_OK;
	int e = MSC_OK;
	if (!rank_lists_ready(ctx, c_sp, &e, rq.close_list.pos != nullptr)) return e;
	if (!ctx->rk_guard) {
		HIP_TRY(ctx, hipHostMalloc((void**)&ctx->rk_guard, 64, hipHostMallocDefault));
		*ctx->rk_guard = 0;
	}
	rt->pass = PASS_RANKS_1XM;
	rt->kernel = "k_pair_ranks_1xm";
	if (long_lists && items_ok) {
		if ((r = rank_multi_ready(ctx, c_sp))) return r;
		rt->pass = PASS_RANKS_ITEMS;
		rt->kernel = "k_pair_ranks_items";
		rt->rank_rounds = (uint32_t)pass_rounds;
	}
	return MSC_OK;
}

// The one place that decides how a call runs -- and that reads MSC_NO_SPARSE_MIRROR, msc_set_mirror_pass, MSC_NO_RANKS_1XM, MSC_NO_RANKS_DIV,
// MSC_RANKS_DIV, MSC_RANKS_ITEMS_FROM, MSC_NO_RANKS_ITEMS and MSC_NO_FUSED_REDUCE. It prepares what the decision depends on (the sparse mirrors,
// the rank lists, which count their requests) and nothing else.
int pick_score_route(msc_ctx* ctx, const ScoreRequest& rq, ScoreRoute* rt) {
	const msc_hist_set* cs = rq.cands;
	const MscLayout& L = cs->L;
	int r;
	rt->nf = __builtin_popcountll(rq.feat_mask);
	rt->ns = rq.model ? rq.model->h.n_singles : 0;
	rt->nc = rq.model ? rq.model->h.n_combos : 0;
	uint64_t want = rq.feat_mask;
	if (rq.model) for (int i = 0; i < rt->ns; i++) want |= rq.model->h.single_flag[i];
	const bool need_div = (want & MSC_FEAT_DIV) != 0 && !rq.only_tiles;
	const bool need_grp = (want & MSC_FEAT_GROUPS) != 0 && !rq.only_tiles;      // sim_mm / rre_k_r: 4-bin group statistics
	const bool wide = needs_wide(rq.cands, rq.qset);
	// The divergence statistics of a DENSE set are scored on its sparse mirror by the same merge kernels a sparse set uses (one
	// evaluation order in every route); the dense streaming kernel then only produces the integer reductions. Histograms too small
	// for the sparse layout (< 64 KiB) keep the table form inside the streaming kernel.
	// r04: a DENSE set's 1 x M pass runs over its sparse mirror too whenever the mirror exists (histograms of 64 KiB and more, narrow
	// range): the merge kernels read 8 bytes per counted k-mer where k_pair_tiles streams 4^k bins (cfg2: ~8 KB against 1 MiB per
	// candidate), and return the same integer reductions bit for bit (test_sparse_sets_equal_dense_sets). The streaming kernel keeps
	// the histograms without a list form, the wide range, and msc_mean_nearest's pass against a mean (only_tiles).
	const bool mirror_pass = !cs->sparse && !wide && !rq.only_tiles && mirror_pass_allowed(ctx, L);
	rt->pass = wide ? PASS_TILES_WIDE : PASS_TILES;
	if (cs->sparse) { rt->c_sp = cs; rt->q_sp = rq.qset; rt->pass = PASS_MERGE; }
	else if (need_div || need_grp || mirror_pass) {
		if ((r = ensure_sparse_mirror(ctx, cs, &rt->c_sp)) || (r = ensure_sparse_mirror(ctx, rq.qset, &rt->q_sp))) return r;
		if (!rt->c_sp || !rt->q_sp) rt->c_sp = rt->q_sp = nullptr;
		if (rt->c_sp && mirror_pass) rt->pass = PASS_MERGE;          // (a padded histogram has no mirror: what exists passes the rule's layout test)
	}
	const msc_hist_set *c_sp = rt->c_sp, *q_sp = rt->q_sp;
	// sim_mm / rre_k_r: from the lists where they exist, else (histograms under 64 KiB) by the dense group kernels -- a given (k, dtype)
	// always takes the same one of the two, so a pair has one evaluation order in every route
	rt->grp = !need_grp ? GRP_NONE : c_sp ? GRP_LISTS : GRP_DENSE;
	if (rt->grp == GRP_DENSE && std::max(rq.cands->max_count, rq.qset->max_count) > 0xffffffffull)
		return fail(ctx, MSC_ERR_UNSUPPORTED, "sim_mm / rre_k_r: counts above 2^32 - 1 are not supported");
	rt->spk = c_sp ? pick_sparse_kernel(c_sp, q_sp, rq.q_slot, std::max(rq.cands->max_count, rq.qset->max_count), wide) : SPK_GENERIC;
	const uint32_t q_nnz = c_sp ? q_sp->hdr_host[rq.q_slot].nnz : 0;
	const bool whole_lists = c_sp && msc_sparse_wl_fits(q_nnz, c_sp->max_nnz);
	rt->kernel = rt->lists() ? (rt->spk == SPK_MP && !need_div && whole_lists ? "k_pair_sparse_wl" : sparse_kernel_name(rt->spk)) : wide ? "k_pair_tiles_wide" : "k_pair_tiles";
	rt->q_kmers = rq.qset->max_sum >= L.nbins ? rq.qset->max_sum - L.nbins : ~0ull;
	if (c_sp && (r = pick_rank_pass(ctx, rq, need_div, rt))) return r;
	// the divergence sums: the mirror may be here for the group statistics alone; without one, the table form inside k_pair_tiles / the direct
	// form inside the wide kernel
	rt->div = !need_div ? DIV_NONE : rt->ranks() ? DIV_RANKS : rt->lists() ? DIV_LISTS : c_sp ? DIV_MIRROR : DIV_INLINE;
	// a sparse set's integer statistics through the merge-path kernel: a short window is shared out, several waves per candidate
	// (never the divergence form: its FP64 sums keep one evaluation order whatever the window)
	// ... and so is the divergence form (sparse sets and the mirror pass of dense ones): its FP64 sums leave per granule of the merged
	// order and are added in granule order by the epilogue, whatever the number of waves that shared a pair
	const uint64_t mp_entries = c_sp ? (uint64_t)q_nnz + c_sp->max_nnz : 0;
	rt->mp_parts = c_sp && !rt->ranks() && rt->spk == SPK_MP && (need_div || (rt->lists() && !whole_lists))
	                   ? msc_sparse_mp_parts((uint32_t)std::min<uint64_t>(rq.m, 0xffffffffu), mp_entries, ctx->num_cus, need_div) : 1;
	rt->SPN = sparse_records(rt->spk, rt->mp_parts);
	rt->DVN = rt->div == DIV_RANKS ? 1 : div_records(rt->spk, mp_entries);
	rt->PS = rt->lists() ? rt->SPN : L.S;
	rt->chunk = std::max<uint64_t>((256ull << 20) / ((uint64_t)rt->PS * sizeof(MscPartial)), 1024);          // the partial records of a chunk stay <= 256 MiB
	if (rq.reduce_mode >= 0 || rq.only_tiles) rt->chunk = rq.m;      // reductions run over the whole window in one piece
	rt->chunk = std::min(rt->chunk, rq.m);
	rt->need_po = rq.sum_out || rq.csum_out || rq.combo0_out || rq.status_out || rq.reduce_mode < 0;
	// a reduced pass that returns nothing per pair: epilogue, first reduce stage and the window's close pass in one kernel
	rt->fused = rq.reduce_mode >= 0 && !rt->need_po && !rq.raw_out && !rq.singles_out && !rq.combos_out && rt->PS <= 4 && getenv("MSC_NO_FUSED_REDUCE") == nullptr;
	return MSC_OK;
}

// ================================================================================================ the stages of a call

// the scratch of a chunk of rt.chunk candidates, the slot list on the device
int ensure_score_scratch(msc_ctx* ctx, const ScoreRequest& rq, const ScoreRoute& rt) {
	const MscLayout& L = rq.cands->L;
	const uint64_t m = rq.m, chunk = rt.chunk;
	int r;
	if ((r = ensure(ctx, ctx->partials, chunk * rt.PS * sizeof(MscPartial)))) return r;
	if (rq.cand_slots && !(rq.slots_uploaded && ctx->slots.cap >= m * sizeof(uint32_t))) {
		if ((r = ensure(ctx, ctx->slots, m * sizeof(uint32_t))) || (r = ensure_pinned(ctx, ctx->pin_up, m * sizeof(uint32_t)))) return r;
		memcpy(ctx->pin_up.p, rq.cand_slots, m * sizeof(uint32_t));      // the previous call's copy has completed: every call ends in a sync
		HIP_TRY(ctx, hipMemcpyAsync(ctx->slots.p, ctx->pin_up.p, m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	}
	// the query's rank list where a rank pass keeps it in global memory
	const uint64_t rk_q_words = rt.pass == PASS_RANKS_ITEMS ? ((rt.q_kmers + 255) & ~255ull) + 256 : rt.pass == PASS_RANKS_1XM ? msc_ranks_pass_query_scratch(rt.q_kmers) : 0;
	if (rk_q_words && (r = ensure(ctx, ctx->rk_q, rk_q_words * sizeof(uint32_t)))) return r;
	// (long lists: a record and a spot-term slot per item, nothing to clear; the pass's counters in two sets used in turn, each pass clearing the other's)
	if (rt.pass == PASS_RANKS_ITEMS) {
		if ((r = ensure(ctx, ctx->rk_acc, msc_ranks_items_rec_bytes(chunk, rt.rank_rounds))) || (r = ensure(ctx, ctx->rk_items, msc_ranks_items_list_bytes(chunk, rt.rank_rounds)))) return r;
		if (!ctx->rk_counters.p) {
			if ((r = ensure(ctx, ctx->rk_counters, 32 * sizeof(uint32_t)))) return r;
			HIP_TRY(ctx, hipMemsetAsync(ctx->rk_counters.p, 0, 32 * sizeof(uint32_t), ctx->stream));
		}
		if (ctx->rk_table_words != msc_ranks_items_table_words(L.nbins)) {          // (another k: both sets start out zero again)
			ctx->rk_table_words = msc_ranks_items_table_words(L.nbins);
			if ((r = ensure(ctx, ctx->rk_tables, 2 * (size_t)ctx->rk_table_words * sizeof(uint32_t)))) return r;
			HIP_TRY(ctx, hipMemsetAsync(ctx->rk_tables.p, 0, 2 * (size_t)ctx->rk_table_words * sizeof(uint32_t), ctx->stream));
		}
	}
	if (rt.div == DIV_RANKS && (r = ensure(ctx, ctx->rk_big, ((size_t)rt.q_sp->hdr_host[rq.q_slot].nnz + 1) * sizeof(uint32_t)))) return r;
	if (rt.div != DIV_NONE) {
		const int tb = msc_div_table_dim(L);
		if (rt.div != DIV_RANKS && (r = ensure(ctx, ctx->div_tables, chunk * (rt.c_sp ? 256 : tb * tb) * 16))) return r;
		if ((r = ensure(ctx, ctx->div_partials, chunk * (rt.c_sp ? rt.DVN : rt.PS) * 16))) return r;
		if (rt.div == DIV_MIRROR && (r = ensure(ctx, ctx->sp_partials, chunk * rt.SPN * sizeof(MscPartial)))) return r;
	}
	if (rt.grp != GRP_NONE) {
		if ((r = ensure(ctx, ctx->grp_pairs, chunk * 32 * sizeof(double)))) return r;
		if ((r = ensure(ctx, ctx->grp_self, (chunk + 1) * 16 * sizeof(double)))) return r;      // [candidates][16] then the query's 16
	}
	if (rq.only_tiles) return MSC_OK;
	if ((r = ensure(ctx, ctx->pair_out, chunk * sizeof(MscPairOut)))) return r;
	if (rq.raw_out && (r = ensure(ctx, ctx->raw, chunk * rt.nf * sizeof(double)))) return r;
	if (rq.singles_out && (r = ensure(ctx, ctx->singles, chunk * rt.ns * sizeof(double)))) return r;
	if (rq.combos_out && (r = ensure(ctx, ctx->combos, chunk * rt.nc * sizeof(double)))) return r;
	if ((r = ensure(ctx, ctx->flags, 64 + chunk))) return r;      // [reduce record (64 B)][close flags]: one copy back
	return ensure(ctx, ctx->reduce_out, sizeof(MscReduceOut));
}

ScoreChunk score_chunk(const msc_ctx* ctx, const ScoreRequest& rq, const ScoreRoute& rt, uint64_t off) {
	const msc_hist_set* cs = rq.cands;
	ScoreChunk ck;
	ck.off = off;
	ck.mc = (uint32_t)std::min(rt.chunk, rq.m - off);
	ck.d_slots = rq.dev_slots ? rq.dev_slots : rq.cand_slots ? (const uint32_t*)ctx->slots.p + off : nullptr;
	ck.c_bins = cs->sparse ? nullptr : cs->bins + (ck.d_slots ? 0 : off * cs->L.slot_bytes);
	ck.c_scal = cs->scalars + (ck.d_slots ? 0 : off * cs->scalar_stride);
	ck.q_bins = cs->sparse ? nullptr : rq.qset->bins + rq.q_slot * rq.qset->L.slot_bytes;
	ck.q_scal = rq.qset->scalars + rq.q_slot * rq.qset->scalar_stride;
	return ck;
}

// the kernel that streams the candidates of a chunk
hipError_t launch_pass_kernel(msc_ctx* ctx, const ScoreRequest& rq, const ScoreRoute& rt, const ScoreChunk& ck) {
	const msc_hist_set *cs = rq.cands, *c_sp = rt.c_sp, *q_sp = rt.q_sp;
	const MscLayout& L = cs->L;
	MscPartial* partials = (MscPartial*)ctx->partials.p;
	switch (rt.pass) {
	case PASS_RANKS_ITEMS: {
		MscRankDiv dv{(uint32_t*)ctx->rk_big.p, ck.q_scal, rq.order, (double*)ctx->div_partials.p};
		return msc_launch_pair_ranks_items(ctx->stream, c_sp->rkl, c_sp->rkl_off, c_sp->rkl_n, c_sp->rkm, c_sp->rkm_off, c_sp->rkm_n, ck.c_scal, cs->scalar_stride, ck.d_slots, ck.off, ck.mc,
		                                         q_sp->ent, q_sp->cum, q_sp->hdr + rq.q_slot, L.nbins, rq.use_window, rq.min_len, rq.max_len, partials, ctx->num_cus, (uint32_t*)ctx->rk_q.p,
		                                         rt.rank_rounds, ctx->rk_acc.p, rt.div == DIV_RANKS ? &dv : nullptr, rt.q_kmers, ctx->rk_guard, ctx->rk_items.p, (uint32_t*)ctx->rk_counters.p,
		                                         (uint32_t*)ctx->rk_tables.p, (int)(ctx->rk_turn++ & 1u),
		                                         q_sp == c_sp && rq.q_slot < c_sp->capacity ? c_sp->rkl + c_sp->rkl_off_host[rq.q_slot] : nullptr);
	}
	case PASS_RANKS_1XM:
		return msc_launch_pair_ranks_1xm(ctx->stream, c_sp->rkl, c_sp->rkl_off, c_sp->rkl_n, ck.c_scal, cs->scalar_stride, ck.d_slots, ck.off, ck.mc, q_sp->ent, q_sp->cum,
		                                       q_sp->hdr + rq.q_slot, L.nbins, rq.use_window, rq.min_len, rq.max_len, partials, ctx->num_cus, rt.q_kmers, ctx->rk_guard, (uint32_t*)ctx->rk_q.p);
	case PASS_MERGE:
		return launch_sparse_pass(ctx, rt.spk, c_sp, cs->scalars, cs->scalar_stride, ck.d_slots, ck.off, ck.mc, q_sp, rq.q_slot, ck.q_scal, L.nbins, rq.use_window, rq.min_len, rq.max_len,
		                                partials, rt.div == DIV_LISTS ? ctx->div_tables.p : nullptr, rt.div == DIV_LISTS ? ctx->div_partials.p : nullptr, rq.order, rt.mp_parts, rt.DVN);
	case PASS_TILES_WIDE:
		return msc_launch_pair_tiles_wide(ctx->stream, L, cs->dtype, ck.c_bins, ck.c_scal, ck.d_slots, ck.mc, ck.q_bins, ck.q_scal, rq.use_window, rq.min_len, rq.max_len, partials,
		                                        ctx->num_cus, rt.div == DIV_INLINE ? ctx->div_partials.p : nullptr, rq.order);
	case PASS_TILES:
		return msc_launch_pair_tiles(ctx->stream, L, cs->dtype, ck.c_bins, ck.c_scal, ck.d_slots, ck.mc, ck.q_bins, ck.q_scal, rq.use_window, rq.min_len, rq.max_len, partials,
		                                   ctx->num_cus, rt.div == DIV_INLINE ? ctx->div_tables.p : nullptr, rt.div == DIV_INLINE ? ctx->div_partials.p : nullptr, rq.order);
	}
	return hipErrorInvalidValue;
}

// ... between the two timing events
int launch_score_pass(msc_ctx* ctx, const ScoreRequest& rq, const ScoreRoute& rt, const ScoreChunk& ck) {
	const msc_hist_set* cs = rq.cands;
	int r;
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles0, ctx->stream));
	if (rt.lists() && g_profile_calls) {
		if (!ctx->prof_nnz.p) { if ((r = ensure(ctx, ctx->prof_nnz, 32))) return r; HIP_TRY(ctx, hipMemsetAsync(ctx->prof_nnz.p, 0, 32, ctx->stream)); }
		HIP_TRY(ctx, msc_launch_sparse_nnz_sum(ctx->stream, rt.c_sp->hdr, cs->scalars, cs->scalar_stride, ck.d_slots, ck.off, ck.mc, rq.use_window, rq.min_len, rq.max_len,
		                                       (uint64_t*)ctx->prof_nnz.p + (rt.ranks() ? 2 : 0)));
		ctx->prof_q_nnz += rt.q_sp->hdr_host[rq.q_slot].nnz;
	}
	HIP_TRY(ctx, launch_pass_kernel(ctx, rq, rt, ck));
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles1, ctx->stream));
	return MSC_OK;
}

// what rides beside the pass (outside its timing): the divergence sums of a streamed chunk from the lists of the same slots, the group statistics
int launch_side_passes(msc_ctx* ctx, const ScoreRequest& rq, const ScoreRoute& rt, const ScoreChunk& ck) {
	const msc_hist_set *cs = rq.cands, *c_sp = rt.c_sp, *q_sp = rt.q_sp;
	double *grp_pairs = (double*)ctx->grp_pairs.p, *grp_self = (double*)ctx->grp_self.p;
	if (rt.div == DIV_MIRROR)
		HIP_TRY(ctx, launch_sparse_pass(ctx, rt.spk, c_sp, cs->scalars, cs->scalar_stride, ck.d_slots, ck.off, ck.mc, q_sp, rq.q_slot, ck.q_scal, cs->L.nbins, rq.use_window, rq.min_len,
		                                rq.max_len, (MscPartial*)ctx->sp_partials.p, ctx->div_tables.p, ctx->div_partials.p, rq.order, rt.mp_parts, rt.DVN));
	if (rt.grp == GRP_DENSE) {
		HIP_TRY(ctx, msc_launch_pair_groups_dense(ctx->stream, cs->L, cs->dtype, ck.c_bins, ck.c_scal, cs->scalar_stride, ck.d_slots, ck.mc, ck.q_bins, rq.use_window, rq.min_len, rq.max_len, grp_pairs));
		HIP_TRY(ctx, msc_launch_self_markov_dense(ctx->stream, cs->L, cs->dtype, cs->bins, ck.d_slots, ck.off, ck.mc, grp_self));
		HIP_TRY(ctx, msc_launch_self_markov_dense(ctx->stream, rq.qset->L, rq.qset->dtype, rq.qset->bins, nullptr, rq.q_slot, 1, grp_self + rt.chunk * 16));
	} else if (rt.grp == GRP_LISTS) {
		HIP_TRY(ctx, msc_launch_pair_sparse_groups(ctx->stream, c_sp->ent, c_sp->hdr + (ck.d_slots ? 0 : ck.off), ck.c_scal, cs->scalar_stride, ck.d_slots, ck.mc, q_sp->ent, q_sp->hdr + rq.q_slot,
		                                           rq.use_window, rq.min_len, rq.max_len, grp_pairs));
		HIP_TRY(ctx, msc_launch_sparse_self_markov(ctx->stream, c_sp->ent, c_sp->hdr, ck.d_slots, ck.off, ck.mc, grp_self));
		HIP_TRY(ctx, msc_launch_sparse_self_markov(ctx->stream, q_sp->ent, q_sp->hdr, nullptr, rq.q_slot, 1, grp_self + rt.chunk * 16));
	}
	return MSC_OK;
}

// the epilogue's arguments for a chunk (one query: the fields of several queries and the error word stay clear, unlike fill_pair_args)
void fill_score_args(MscEpilogueArgs& ea, const msc_ctx* ctx, const ScoreRequest& rq, const ScoreRoute& rt, const ScoreChunk& ck) {
	const msc_hist_set* cs = rq.cands;
	memset(&ea, 0, sizeof ea);
	ea.partials = (const MscPartial*)ctx->partials.p;
	if (rt.div == DIV_INLINE) ea.div_partials = ctx->div_partials.p;
	else if (rt.div != DIV_NONE) { ea.div_direct = (const double*)ctx->div_partials.p; ea.div_direct_n = rt.DVN; ea.div_base = cs->L.nbins; }
	if (rt.grp != GRP_NONE) { ea.grp_pairs = (const double*)ctx->grp_pairs.p; ea.grp_self_c = (const double*)ctx->grp_self.p; ea.grp_self_q = ea.grp_self_c + rt.chunk * 16; }
	ea.S = rt.PS; ea.sparse_base = rt.lists() ? cs->L.nbins : 0; ea.m = ck.mc;
	ea.cand_scalars = ck.c_scal; ea.cand_scalar_stride = cs->scalar_stride; ea.cand_slots = ck.d_slots; ea.q_scalars = ck.q_scal;
	ea.nbins = cs->L.nbins; ea.dtype = cs->dtype; ea.order = rq.order;
	ea.use_window = rq.use_window; ea.min_len = rq.min_len; ea.max_len = rq.max_len;
	ea.feat_mask = rq.feat_mask; ea.model = rq.model ? rq.model->d : nullptr;
	ea.raw_out = rq.raw_out ? (double*)ctx->raw.p : nullptr;
	ea.singles_out = rq.singles_out ? (double*)ctx->singles.p : nullptr;
	ea.combos_out = rq.combos_out ? (double*)ctx->combos.p : nullptr;
	ea.pair_out = rt.fused ? nullptr : (MscPairOut*)ctx->pair_out.p;
}

// epilogue, then the reduction where the call asks for one -- or both in the fused kernel
int launch_epilogue_reduce(msc_ctx* ctx, const ScoreRequest& rq, const ScoreRoute& rt, const ScoreChunk& ck, const MscEpilogueArgs& ea, ScoreHome* home) {
	int r;
	if (!rt.fused) HIP_TRY(ctx, msc_launch_epilogue(ctx->stream, ea));
	if (rq.reduce_mode < 0) return MSC_OK;
	// the reduce kernel writes its record and the close flags straight into page-locked host memory the device can address
	// (no copy command behind the kernel): [reduce record (64 B)][close flags]
	constexpr size_t kRo = 64;
	static_assert(sizeof(MscReduceOut) <= kRo, "the reduce record sits in front of the flags");
	if ((r = ensure_pinned(ctx, ctx->pin_down, kRo + ck.mc))) return r;
	uint8_t* down = nullptr;
	HIP_TRY(ctx, hipHostGetDevicePointer((void**)&down, ctx->pin_down.p, 0));
	if ((r = ensure(ctx, ctx->reduce_parts, msc_reduce_scratch_bytes()))) return r;
	uint8_t* d_flags = rq.dev_flags_out ? rq.dev_flags_out : rq.flags_out ? down + kRo : nullptr;
	if (!rt.fused) {
		HIP_TRY(ctx, msc_launch_reduce(ctx->stream, (const MscPairOut*)ctx->pair_out.p, ck.mc, rq.reduce_mode, rq.reduce_begin, d_flags, (MscReduceOut*)down, ctx->reduce_parts.p,
		                               rq.reduce_mode == MSC_REDUCE_GET_CLOSE ? rq.close_list.pos : nullptr));          // (a window pass: ties by window position)
		if (rq.after_reduce) HIP_TRY(ctx, rq.after_reduce((const MscReduceOut*)down));
		return MSC_OK;
	}
	// (the step-serial loop's own call: the workgroups' parts go to page-locked memory and are folded by the host, behind the wait for the
	// stream -- k_pair_reduce_fold2 was one of a pass's launches)
	ReducePart* host_parts = nullptr;
	if (rq.close_list.pos && rq.close_list.out_host && ck.off == 0 && ck.mc == rq.m) {
		if ((r = ensure_pinned(ctx, ctx->pin_parts, 1024 * sizeof(ReducePart)))) return r;
		HIP_TRY(ctx, hipHostGetDevicePointer((void**)&host_parts, ctx->pin_parts.p, 0));
	}
	home->fold_on_host = host_parts != nullptr;
	HIP_TRY(ctx, msc_launch_epilogue_reduce(ctx->stream, ea, rq.reduce_mode, rq.reduce_begin, d_flags, (MscReduceOut*)down, ctx->reduce_parts.p, rq.close_list, host_parts, &home->n_parts));
	if (rq.after_reduce && !rq.close_list.pos) HIP_TRY(ctx, rq.after_reduce((const MscReduceOut*)down));
	return MSC_OK;
}

// the chunk's results home: the copies, the call's one wait for the stream, the host's fold of the reduction, the per-pair records scattered
int bring_home(msc_ctx* ctx, const ScoreRequest& rq, const ScoreRoute& rt, const ScoreChunk& ck, ScoreHome* home, double t_issue) {
	const uint64_t off = ck.off;
	const uint32_t mc = ck.mc;
	if (rq.raw_out) HIP_TRY(ctx, hipMemcpyAsync(rq.raw_out + off * rt.nf, ctx->raw.p, (size_t)mc * rt.nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (rq.singles_out) HIP_TRY(ctx, hipMemcpyAsync(rq.singles_out + off * rt.ns, ctx->singles.p, (size_t)mc * rt.ns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (rq.combos_out) HIP_TRY(ctx, hipMemcpyAsync(rq.combos_out + off * rt.nc, ctx->combos.p, (size_t)mc * rt.nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (rt.need_po) {
		home->po.resize(mc);
		HIP_TRY(ctx, hipMemcpyAsync(home->po.data(), ctx->pair_out.p, (size_t)mc * sizeof(MscPairOut), hipMemcpyDeviceToHost, ctx->stream));
	}
	const double t_wait = g_profile_calls ? now_s() : 0;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (g_profile_calls) { ctx->prof_issue += t_wait - t_issue; ctx->prof_wait += now_s() - t_wait; }
	if (rq.reduce_mode >= 0) {
		if (home->fold_on_host) {
			uint32_t wpos = 0;
			msc_reduce_fold_host((const ReducePart*)ctx->pin_parts.p, home->n_parts, rq.reduce_mode, rq.reduce_host, &wpos);
			rq.close_list.out_host[0] = wpos;
		} else memcpy(rq.reduce_host, ctx->pin_down.p, sizeof(MscReduceOut));
		if (rq.flags_out) memcpy(rq.flags_out, (const uint8_t*)ctx->pin_down.p + 64, mc);
	}
	float t = 0;
	if (ctx->timing && hipEventElapsedTime(&t, ctx->ev_tiles0, ctx->ev_tiles1) == hipSuccess) { ctx->tiles_ms_accum += t; ctx->tiles_launches++; ctx->have_timing = true; }
	if (!rt.need_po) return MSC_OK;
	for (uint32_t i = 0; i < mc; i++) {
		const MscPairOut& p = home->po[i];
		if (rq.sum_out) rq.sum_out[off + i] = p.sum;
		if (rq.csum_out) rq.csum_out[off + i] = p.csum;
		if (rq.combo0_out) rq.combo0_out[off + i] = p.combo0;
		if (rq.status_out) rq.status_out[off + i] = p.status;
		if (rq.flags_out && rq.reduce_mode < 0) rq.flags_out[off + i] = (p.status == 0 && p.close) ? 1 : 0;
		if (p.status < 0 && p.status < home->first_err) home->first_err = p.status;
	}
	return MSC_OK;
}

}  // namespace

// One 1 x M call: streams the candidates once, then folds / evaluates per candidate, chunk by chunk.
int run_score(msc_ctx* ctx, ScoreRequest& rq) {
	const double t_call = g_profile_calls ? now_s() : 0;
	int r = validate_pair(ctx, rq.cands, rq.qset, rq.q_slot, rq.cand_slots, rq.dev_slots ? 0 : rq.m);
	if (r) return r;
	if (rq.dev_slots && (rq.cand_slots || rq.reduce_mode < 0 || rq.m > 0xfffffff0ull)) return fail(ctx, MSC_ERR_INVALID_ARG, "run_score: a device slot list goes with a reduction only");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	ctx->tiles_ms_accum = 0.f;
	ctx->tiles_launches = 0;
	ctx->have_timing = false;
	ctx->last_kernel = rq.cands->sparse ? "k_pair_sparse" : needs_wide(rq.cands, rq.qset) ? "k_pair_tiles_wide" : "k_pair_tiles";
	ctx->last_query_tile = 1;
	if (rq.m == 0) {
		const bool gc = rq.reduce_mode == MSC_REDUCE_GET_CLOSE;
		if (rq.reduce_host) *rq.reduce_host = MscReduceOut{gc ? -1.0 : DBL_MIN, gc ? -1 : 0, 0, 0, 0};
		return MSC_OK;
	}
	ScoreRoute rt;
	if ((r = pick_score_route(ctx, rq, &rt))) return r;
	ctx->last_kernel = rt.kernel;
	ctx->last_partial_stride = rt.PS;
	if ((r = ensure_score_scratch(ctx, rq, rt))) return r;
	ScoreHome home;
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all0, ctx->stream));
	if (g_profile_calls) { ctx->prof_calls++; ctx->prof_cands += rq.m; ctx->prof_prep += now_s() - t_call; }
	for (uint64_t off = 0; off < rq.m; off += rt.chunk) {
		const double t_issue = g_profile_calls ? now_s() : 0;
		const ScoreChunk ck = score_chunk(ctx, rq, rt, off);
		if ((r = launch_score_pass(ctx, rq, rt, ck)) || (r = launch_side_passes(ctx, rq, rt, ck))) return r;
		if (!rq.only_tiles) {
			MscEpilogueArgs ea;
			fill_score_args(ea, ctx, rq, rt, ck);
			if ((r = launch_epilogue_reduce(ctx, rq, rt, ck, ea, &home))) return r;
		}
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all1, ctx->stream));
		if (rq.only_tiles) return MSC_OK;          // (one chunk; msc_mean_nearest folds the partial records itself)
		if ((r = bring_home(ctx, rq, rt, ck, &home, t_issue))) return r;
	}
	if (rt.ranks() && *ctx->rk_guard) {
		*ctx->rk_guard = 0;
		return fail(ctx, MSC_ERR_HIP, "rank pass: the query's list is longer than its set's bound (max_sum not maintained by a writer of that set)");
	}
	if (rq.reduce_host && rq.reduce_host->first_error < home.first_err) home.first_err = rq.reduce_host->first_error;
	return pair_status(ctx, home.first_err);
}


// members against their rounded mean in slot 0 of rs: the pass alone (only the |p - r| reduction is used; the slots are in ctx->slots already)
static int score_against_mean(msc_ctx* ctx, const msc_hist_set* set, const uint32_t* member_slots, uint64_t m, const msc_hist_set* rs) {
	ScoreRequest rq;
	rq.cands = set; rq.cand_slots = member_slots; rq.m = m; rq.qset = rs; rq.q_slot = 0; rq.only_tiles = true;
	rq.slots_uploaded = member_slots != nullptr;
	return run_score(ctx, rq);
}

extern "C" int msc_pair_features_raw(msc_ctx* ctx, const msc_hist_set* cands, const uint32_t* cand_slots, uint64_t m, const msc_hist_set* qset,
                                     uint64_t q_slot, int order, uint64_t feat_mask, double* raw_out) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (!raw_out && m) return fail(ctx, MSC_ERR_INVALID_ARG, "raw_out is NULL");
	if (feat_mask == 0 || (feat_mask & ~kSupportedFeats))
		return fail(ctx, MSC_ERR_UNSUPPORTED, "feat_mask 0x%llx holds statistics outside the GPU path (supported 0x%llx)", (unsigned long long)feat_mask,
		            (unsigned long long)kSupportedFeats);
	ScoreRequest rq;
	rq.cands = cands; rq.cand_slots = cand_slots; rq.m = m; rq.qset = qset; rq.q_slot = q_slot; rq.order = order;
	rq.feat_mask = feat_mask; rq.raw_out = raw_out;
	return run_score(ctx, rq);
}

extern "C" int msc_score(msc_ctx* ctx, const msc_model* model, const msc_hist_set* cands, const uint32_t* cand_slots, uint64_t m,
                         const msc_hist_set* qset, uint64_t q_slot, int order, double* singles_out, double* combos_out, double* sum_out,
                         double* csum_out) {
	if (!ctx || !model || model->ctx != ctx) return MSC_ERR_INVALID_ARG;
	ScoreRequest rq;
	rq.model = model; rq.cands = cands; rq.cand_slots = cand_slots; rq.m = m; rq.qset = qset; rq.q_slot = q_slot; rq.order = order;
	rq.singles_out = singles_out; rq.combos_out = combos_out; rq.sum_out = sum_out; rq.csum_out = csum_out;
	return run_score(ctx, rq);
}

extern "C" int msc_get_close(msc_ctx* ctx, const msc_model* model, double cutoff, const msc_hist_set* cands, const uint32_t* cand_slots,
                             uint64_t m, const msc_hist_set* qset, uint64_t q_slot, uint8_t* close_flags, int64_t* best_pos, double* best_sim,
                             int* is_min) {
	if (!ctx || !model || model->ctx != ctx || !qset) return MSC_ERR_INVALID_ARG;
	if (m && !close_flags) return fail(ctx, MSC_ERR_INVALID_ARG, "close_flags is NULL");
	int r = check_slot(ctx, qset, q_slot);
	if (r) return r;
	uint64_t q_len = 0;
	if ((r = slot_length(ctx, qset, q_slot, &q_len))) return r;
	ScoreRequest rq;
	rq.model = model; rq.cands = cands; rq.cand_slots = cand_slots; rq.m = m; rq.qset = qset; rq.q_slot = q_slot;
	rq.order = MSC_ORDER_CAND_FIRST;                              // feat->compute(*pt, *p), cluster/Trainer.cpp:49
	rq.use_window = 1;
	rq.min_len = (uint64_t)((double)q_len * cutoff);              // uint64_t min_len = p->get_length() * cutoff;  :39
	rq.max_len = (uint64_t)((double)q_len / cutoff);              // uint64_t max_len = p->get_length() / cutoff;  :40
	rq.flags_out = close_flags;
	rq.reduce_mode = MSC_REDUCE_GET_CLOSE;
	MscReduceOut ro;
	memset(&ro, 0, sizeof ro);
	rq.reduce_host = &ro;
	if ((r = run_score(ctx, rq))) return r;
	if (best_pos) *best_pos = ro.best_pos;
	if (best_sim) *best_sim = ro.best_sim;
	if (is_min) *is_min = ro.any_close ? 0 : 1;
	return MSC_OK;
}

extern "C" int msc_filter(msc_ctx* ctx, const msc_model* model, double cutoff, const msc_hist_set* centre_set, uint64_t centre_slot,
                          const msc_hist_set* pts, const uint32_t* pt_slots, uint64_t m, uint8_t* keep, uint64_t* n_kept) {
	if (!ctx || !model || model->ctx != ctx || !centre_set) return MSC_ERR_INVALID_ARG;
	if (m && !keep) return fail(ctx, MSC_ERR_INVALID_ARG, "keep is NULL");
	int r = check_slot(ctx, centre_set, centre_slot);
	if (r) return r;
	uint64_t c_len = 0;
	if ((r = slot_length(ctx, centre_set, centre_slot, &c_len))) return r;
	ScoreRequest rq;
	rq.model = model; rq.cands = pts; rq.cand_slots = pt_slots; rq.m = m; rq.qset = centre_set; rq.q_slot = centre_slot;
	rq.order = MSC_ORDER_QUERY_FIRST;                             // classify(p, pt.first), cluster/Trainer.cpp:133
	rq.use_window = 1;
	rq.min_len = (uint64_t)((double)c_len * trainer_get_id(cutoff));          // :126-127
	rq.max_len = (uint64_t)((double)c_len / trainer_get_id(cutoff));
	rq.flags_out = keep;                                          // kept  <=>  in window && round(classify) != 0
	if ((r = run_score(ctx, rq))) return r;
	if (n_kept) { uint64_t n = 0; for (uint64_t i = 0; i < m; i++) n += keep[i]; *n_kept = n; }
	return MSC_OK;
}

extern "C" int msc_merge(msc_ctx* ctx, const msc_model* model, double cutoff, const msc_hist_set* centres, const uint32_t* centre_slots,
                         uint64_t n, int64_t current, int64_t begin, int64_t last, int64_t* best_out) {
	if (!ctx || !model || model->ctx != ctx || !centres || !best_out) return MSC_ERR_INVALID_ARG;
	if (current < 0 || (uint64_t)current >= n) return fail(ctx, MSC_ERR_INVALID_ARG, "current out of range");
	*best_out = 0;
	if (begin > last) return MSC_OK;
	if (begin < 0 || (uint64_t)last >= n) return fail(ctx, MSC_ERR_INVALID_ARG, "[begin,last] out of range");
	const uint64_t cur_slot = centre_slots ? centre_slots[current] : (uint64_t)current;
	int r = check_slot(ctx, centres, cur_slot);
	if (r) return r;
	uint64_t c_len = 0;
	if ((r = slot_length(ctx, centres, cur_slot, &c_len))) return r;
	std::vector<uint32_t> slots((size_t)(last - begin + 1));
	for (int64_t i = begin; i <= last; i++) slots[(size_t)(i - begin)] = centre_slots ? centre_slots[i] : (uint32_t)i;
	std::vector<uint8_t> flags(slots.size());
	ScoreRequest rq;
	rq.model = model; rq.cands = centres; rq.cand_slots = slots.data(); rq.m = slots.size(); rq.qset = centres; rq.q_slot = cur_slot;
	rq.order = MSC_ORDER_CAND_FIRST;                              // feat->compute(*cen, *p), cluster/Trainer.cpp:93
	rq.use_window = 1;
	rq.min_len = (uint64_t)((double)c_len * trainer_get_id(cutoff));
	rq.max_len = (uint64_t)((double)c_len / trainer_get_id(cutoff));
	rq.flags_out = flags.data();
	rq.reduce_mode = MSC_REDUCE_MERGE;
	rq.reduce_begin = begin;
	MscReduceOut ro;
	memset(&ro, 0, sizeof ro);
	rq.reduce_host = &ro;
	if ((r = run_score(ctx, rq))) return r;
	*best_out = ro.best_pos;
	return MSC_OK;
}

extern "C" int msc_search(msc_ctx* ctx, const msc_model* cls, const msc_model* reg, const msc_hist_set* db, const uint32_t* db_slots,
                          uint64_t m, const msc_hist_set* qset, uint64_t q_slot, uint8_t* close_out, double* sim_out) {
	if (!ctx || (cls && cls->ctx != ctx) || (reg && reg->ctx != ctx)) return MSC_ERR_INVALID_ARG;
	if (!cls && !reg) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_search needs a classification or a regression model");
	// work() follows pred->get_mode() (fastcar/FC_Runner.cpp:432,446-458): without a classification block every pair of the
	// window counts as close, without a regression block the similarity of a close pair is 1
	int r;
	if (cls) {
		// pred->close(pts[i], query) then pred->similarity(pts[i], query): fastcar/FC_Runner.cpp:449-455
		ScoreRequest a;
		a.model = cls; a.cands = db; a.cand_slots = db_slots; a.m = m; a.qset = qset; a.q_slot = q_slot; a.order = MSC_ORDER_CAND_FIRST;
		a.flags_out = close_out;
		if ((r = run_score(ctx, a))) return r;
	} else {
		if ((r = validate_pair(ctx, db, qset, q_slot, db_slots, m))) return r;
		if (close_out) memset(close_out, 1, m);
	}
	if (reg && sim_out) {
		ScoreRequest b;
		b.model = reg; b.cands = db; b.cand_slots = db_slots; b.m = m; b.qset = qset; b.q_slot = q_slot; b.order = MSC_ORDER_CAND_FIRST;
		b.sum_out = sim_out;
		if ((r = run_score(ctx, b))) return r;
		for (uint64_t i = 0; i < m; i++) {           // p_predict clamps to [0,1], predict/Predictor.cpp:293-298
			if (sim_out[i] < 0) sim_out[i] = 0; else if (sim_out[i] > 1) sim_out[i] = 1;
		}
	} else if (sim_out) {
		for (uint64_t i = 0; i < m; i++) sim_out[i] = 1.0;
	}
	return MSC_OK;
}

// ================================================================================================ mean + nearest

// msc_mean_nearest for sparse members (kernels and the derivation in sparse.hip)
namespace {
__global__ void k_put_words(uint32_t* __restrict__ a, const uint32_t* __restrict__ a_src, uint32_t na, uint32_t* __restrict__ b, const uint32_t* __restrict__ b_src, uint32_t nb) {
	for (uint32_t i = threadIdx.x; i < na; i += blockDim.x) a[i] = a_src[i];
	for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) b[i] = b_src[i];
}
}  // namespace
static int mean_nearest_sparse(msc_ctx* ctx, const msc_hist_set* set, const uint32_t* member_slots, uint64_t m, int64_t* nearest_pos, double* dist_out,
                               double* mean_out) {
	if (mean_out) return fail(ctx, MSC_ERR_UNSUPPORTED, "mean_out is not available for sparse sets");
	if (m > 0xfffffff0ull) return MSC_ERR_INVALID_ARG;
	if (member_slots) { for (uint64_t i = 0; i < m; i++) if (member_slots[i] >= set->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "member slot out of range"); }
	else if (m > set->capacity) return MSC_ERR_INVALID_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const MscLayout& L = set->L;
	int r;
	if (ctx->sp_acc_bins != L.nbins) {          // dense u32 accumulator, zero between calls
		if ((r = ensure(ctx, ctx->sp_acc, L.nbins * sizeof(uint32_t)))) return r;
		HIP_TRY(ctx, hipMemsetAsync(ctx->sp_acc.p, 0, L.nbins * sizeof(uint32_t), ctx->stream));
		ctx->sp_acc_bins = L.nbins;
	}
	uint64_t upper = 0;                           // the rounded mean cannot have more stored bins than the members together
	for (uint64_t i = 0; i < m; i++) upper += set->hdr_host[member_slots ? member_slots[i] : i].nnz;
	upper = std::min<uint64_t>(upper, L.nbins);
	if (!ctx->sparse_mean_set || ctx->sparse_mean_set->k != set->k || ctx->sparse_mean_set->dtype != set->dtype || ctx->sparse_mean_set->ent_capacity < upper + 1) {
		if (ctx->sparse_mean_set) { msc_hist_set_destroy(ctx->sparse_mean_set); ctx->sparse_mean_set = nullptr; }
		if ((r = msc_hist_set_create_sparse(ctx, set->k, set->dtype, 1, std::max<uint64_t>(upper + 1, 1 << 16), &ctx->sparse_mean_set))) return r;
	}
	msc_hist_set* rs = ctx->sparse_mean_set;
	const uint32_t n_chunks = (uint32_t)std::min<uint64_t>(1024, L.nbins / 256);      // multiple of 16 for every k >= 6
	const uint64_t chunk_bins = L.nbins / n_chunks;
	// r05: what the call hands to and fro in small pieces -- the chunk counts (device -> host), the chunks' offsets and running sums,
	// the floor sum, the mean's header and scalar record (host -> device), the reduce record (device -> host) -- sits in ONE page-locked
	// block the kernels address directly; eight staged copies of a few bytes to a few KiB each were a quarter of a `closest` call
	// (cfg5's shape: 141 us per call, 2.5 s of the run). Only the header and the scalar record, which the set's own arrays must hold,
	// and the member slots are still copied (from page-locked memory: no staging).
	struct PinLayout { size_t counts, off, cb, floor_sum, ro, hdr, sc, slots, bytes; } pl;
	pl.counts = 0;
	pl.off = pl.counts + (size_t)n_chunks * 3 * sizeof(uint64_t);
	pl.cb = pl.off + (size_t)n_chunks * sizeof(uint64_t);
	pl.floor_sum = pl.cb + (size_t)n_chunks * sizeof(uint64_t);
	pl.ro = pl.floor_sum + 64;
	pl.hdr = pl.ro + 64;
	pl.sc = pl.hdr + ((sizeof(MscSparseHdr) + 63) & ~(size_t)63);
	pl.slots = pl.sc + ((sizeof(MscSlotScalars) + 63) & ~(size_t)63);
	pl.bytes = pl.slots + (member_slots ? m * sizeof(uint32_t) : 0);
	if ((r = ensure_pinned(ctx, ctx->pin_mean, pl.bytes))) return r;
	uint8_t *pin_h = (uint8_t*)ctx->pin_mean.p, *pin_d = nullptr;
	HIP_TRY(ctx, hipHostGetDevicePointer((void**)&pin_d, ctx->pin_mean.p, 0));
	if (member_slots) {
		if ((r = ensure(ctx, ctx->slots, m * sizeof(uint32_t)))) return r;
		memcpy(pin_h + pl.slots, member_slots, m * sizeof(uint32_t));          // (the previous call's copy has completed: every call ends in a wait for the stream)
		HIP_TRY(ctx, hipMemcpyAsync(ctx->slots.p, pin_h + pl.slots, m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	}
	const uint32_t* d_slots = member_slots ? (const uint32_t*)ctx->slots.p : nullptr;
	uint64_t* d_counts = (uint64_t*)(pin_d + pl.counts);
	// the sweeps of the batched form with one centre of m members; k >= 11: the scatter of that form as well, which marks the 64-byte
	// lines it touches for the sweeps to visit those only
	static const bool no_groups = getenv("MSC_SPARSE_MEAN_NO_GROUPS") != nullptr;
	const bool grouped = !no_groups && L.nbins >= msc_sparse_groups_min_bins() && chunk_bins % 512 == 0 && member_slots;
	uint32_t* touched = nullptr;
	if (grouped) {
		const size_t tb = (size_t)(L.nbins >> 9) * sizeof(uint32_t);
		if (tb > ctx->sp_touched.cap) {
			if ((r = ensure(ctx, ctx->sp_touched, tb))) return r;
			HIP_TRY(ctx, hipMemsetAsync(ctx->sp_touched.p, 0, ctx->sp_touched.cap, ctx->stream));
		}
		touched = (uint32_t*)ctx->sp_touched.p;
		if ((r = ensure(ctx, ctx->pair_seg, m * sizeof(uint32_t)))) return r;
		HIP_TRY(ctx, hipMemsetAsync(ctx->pair_seg.p, 0, m * sizeof(uint32_t), ctx->stream));
		HIP_TRY(ctx, msc_launch_sparse_scatter_batch(ctx->stream, set->ent, set->hdr, d_slots, (const uint32_t*)ctx->pair_seg.p, (uint32_t)m, L.nbins, (uint32_t*)ctx->sp_acc.p,
		                                             touched));
	} else {
		HIP_TRY(ctx, msc_launch_sparse_scatter(ctx->stream, set->ent, set->hdr, d_slots, (uint32_t)m, (uint32_t*)ctx->sp_acc.p));
	}
	HIP_TRY(ctx, msc_launch_sparse_mean_count_batch(ctx->stream, (const uint32_t*)ctx->sp_acc.p, L.nbins, n_chunks, chunk_bins, 1, nullptr, (uint32_t)m, d_counts, touched));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	const uint64_t* counts = (const uint64_t*)(pin_h + pl.counts);
	uint64_t *off = (uint64_t*)(pin_h + pl.off), *cb = (uint64_t*)(pin_h + pl.cb);
	MscSparseHdr h{};
	uint64_t n = 0, ex = 0, fl = 0;
	const uint32_t per_sub = n_chunks / MSC_SPARSE_SUB;
	for (uint32_t c = 0; c < n_chunks; c++) {
		if (c % per_sub == 0) h.split[c / per_sub] = (uint32_t)n;
		off[c] = n;
		cb[c] = ex;
		n += counts[c * 3ull]; ex += counts[c * 3ull + 1]; fl += counts[c * 3ull + 2];
	}
	h.split[MSC_SPARSE_SUB] = (uint32_t)n;
	h.nnz = (uint32_t)n;
	h.off = 0;
	rs->ent_used = n;
	rs->hdr_host[0] = h;
	lists_written(rs, 0, 1);
	rs->max_nnz = std::max(rs->max_nnz, h.nnz);          // (every writer of hdr_host keeps max_nnz >= each list: the whole-list kernel sizes its LDS by it)
	MscSlotScalars sc;
	memset(&sc, 0, sizeof sc);
	sc.sum = L.nbins + ex;          // sum of the rounded mean's bins
	rs->max_sum = std::max<uint64_t>(rs->max_sum, sc.sum);
	sc.mag = sc.sum;
	sc.length = 1;
	*(uint64_t*)(pin_h + pl.floor_sum) = L.nbins + fl;
	memcpy(pin_h + pl.hdr, &h, sizeof h);
	memcpy(pin_h + pl.sc, &sc, sizeof sc);
	// (the header and the scalar record into the set's own arrays by ONE small kernel that reads the page-locked block: two staged copies
	// of a few dozen bytes were 9 us of blit kernels per call, a fifth of the call's kernel time)
	static_assert(sizeof(MscSparseHdr) % 4 == 0 && sizeof(MscSlotScalars) % 4 == 0, "copied word by word");
	k_put_words<<<dim3(1), dim3(64), 0, ctx->stream>>>((uint32_t*)rs->hdr, (const uint32_t*)(pin_d + pl.hdr), (uint32_t)(sizeof h / 4), (uint32_t*)rs->scalars,
	                                                  (const uint32_t*)(pin_d + pl.sc), (uint32_t)(sizeof sc / 4));
	HIP_TRY(ctx, hipGetLastError());
	const uint64_t *d_off = (const uint64_t*)(pin_d + pl.off), *d_cb = (const uint64_t*)(pin_d + pl.cb), *d_floor = (const uint64_t*)(pin_d + pl.floor_sum);
	HIP_TRY(ctx, msc_launch_sparse_mean_write_batch(ctx->stream, (uint32_t*)ctx->sp_acc.p, L.nbins, n_chunks, chunk_bins, 1, nullptr, (uint32_t)m, d_off, d_cb, rs->ent, rs->cum,
	                                                touched));
	if ((r = score_against_mean(ctx, set, member_slots, m, rs))) return r;
	if ((r = ensure(ctx, ctx->raw, m * sizeof(double)))) return r;
	HIP_TRY(ctx, msc_launch_distance_d(ctx->stream, (const MscPartial*)ctx->partials.p, ctx->last_partial_stride, (uint32_t)m, set->scalars, set->scalar_stride, d_slots,
	                                   rs->scalars, d_floor, (double*)ctx->raw.p, (MscReduceOut*)(pin_d + pl.ro)));
	if (dist_out) HIP_TRY(ctx, hipMemcpyAsync(dist_out, ctx->raw.p, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	*nearest_pos = ((const MscReduceOut*)(pin_h + pl.ro))->best_pos;
	return MSC_OK;
}

extern "C" int msc_mean_nearest(msc_ctx* ctx, const msc_hist_set* set, const uint32_t* member_slots, uint64_t m, int64_t* nearest_pos,
                                double* dist_out, double* mean_out) {
	if (!ctx || !set || set->ctx != ctx || !nearest_pos) return MSC_ERR_INVALID_ARG;
	if (m == 0) return fail(ctx, MSC_ERR_INVALID_ARG, "N cannot be 0 (cluster/ClusterFactory.cpp:346-348 throws)");
	if (set->sparse) return mean_nearest_sparse(ctx, set, member_slots, m, nearest_pos, dist_out, mean_out);
	if (m > 0xfffffff0ull) return MSC_ERR_INVALID_ARG;
	if (member_slots) { for (uint64_t i = 0; i < m; i++) if (member_slots[i] >= set->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "member slot out of range"); }
	else if (m > set->capacity) return MSC_ERR_INVALID_ARG;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int r;
	if (!ctx->scratch_set || ctx->scratch_set->k != set->k || ctx->scratch_set->dtype != set->dtype) {
		if (ctx->scratch_set) { msc_hist_set_destroy(ctx->scratch_set); ctx->scratch_set = nullptr; }
		if ((r = msc_hist_set_create(ctx, set->k, set->dtype, 1, &ctx->scratch_set))) return r;
	}
	msc_hist_set* rs = ctx->scratch_set;
	const MscLayout& L = set->L;
	if ((r = ensure(ctx, ctx->floor_sum, 8))) return r;
	if (mean_out && (r = ensure(ctx, ctx->mean, L.padded_bins * sizeof(double)))) return r;
	if (member_slots) {
		if ((r = ensure(ctx, ctx->slots, m * sizeof(uint32_t)))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->slots.p, member_slots, m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	}
	const uint32_t* d_slots = member_slots ? (const uint32_t*)ctx->slots.p : nullptr;
	HIP_TRY(ctx, msc_launch_colsum(ctx->stream, L, set->dtype, set->bins, d_slots, (uint32_t)m, rs->bins, mean_out ? (double*)ctx->mean.p : nullptr,
	                               (uint64_t*)ctx->floor_sum.p, nullptr));
	HIP_TRY(ctx, hipMemsetAsync(rs->scalars, 0, sizeof(MscSlotScalars), ctx->stream));
	if ((r = ensure(ctx, ctx->tile_scratch, (size_t)L.S * 2 * sizeof(uint64_t)))) return r;
	HIP_TRY(ctx, msc_launch_finalize(ctx->stream, rs->bins, rs->scalars, L, set->dtype, 0, 1, false, (uint64_t*)ctx->tile_scratch.p));      // one wave per tile
	if ((r = refresh_bounds(ctx, rs, 0, 1))) return r;
	if ((r = score_against_mean(ctx, set, member_slots, m, rs))) return r;
	if ((r = ensure(ctx, ctx->reduce_out, sizeof(MscReduceOut)))) return r;
	if ((r = ensure(ctx, ctx->raw, m * sizeof(double)))) return r;
	HIP_TRY(ctx, msc_launch_distance_d(ctx->stream, (const MscPartial*)ctx->partials.p, L.S, (uint32_t)m, set->scalars, set->scalar_stride, d_slots,
	                                   rs->scalars, (const uint64_t*)ctx->floor_sum.p, (double*)ctx->raw.p, (MscReduceOut*)ctx->reduce_out.p));
	MscReduceOut ro;
	HIP_TRY(ctx, hipMemcpyAsync(&ro, ctx->reduce_out.p, sizeof ro, hipMemcpyDeviceToHost, ctx->stream));
	if (dist_out) HIP_TRY(ctx, hipMemcpyAsync(dist_out, ctx->raw.p, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (mean_out) {
		if ((r = ensure(ctx, ctx->nat, L.padded_bins * sizeof(double)))) return r;
		MscLayout L64 = L;       // move 8-byte elements through the same bin permutation
		HIP_TRY(ctx, msc_launch_permute(ctx->stream, ctx->mean.p, ctx->nat.p, L64, 64, false));
		HIP_TRY(ctx, hipMemcpyAsync(mean_out, ctx->nat.p, L.nbins * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	float t = 0;
	if (ctx->timing && hipEventElapsedTime(&t, ctx->ev_tiles0, ctx->ev_tiles1) == hipSuccess) { ctx->tiles_ms_accum = t; ctx->tiles_launches = 1; ctx->have_timing = true; }
	*nearest_pos = ro.best_pos;
	return MSC_OK;
}

