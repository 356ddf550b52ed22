// msc_api_multi.hip -- msc_score_multi, the Q x M all-pairs call (fastcar's loop, fastcar/FC_Runner.cpp:426-471): the block plan, a route per
// block, one function per route and, for the matrix cores, one per stage of the block pipe over three streams (the stage decisions themselves are
// plain arithmetic in msc_multi_plan.h). The mirrors of a set it reads (digest, presence bits, ranks) are built in msc_mirrors.hip. Split from
// msc_api.hip in r05.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "msc_internal.h"
#include "msc_fold.h"

#include "msc_objects.h"
#include "msc_api_private.h"


// the epilogue's error word (the stream is idle)
int read_error_word(msc_ctx* ctx) {
	int32_t first_err = 0;
	HIP_TRY(ctx, hipMemcpy(&first_err, ctx->err_word.p, sizeof first_err, hipMemcpyDeviceToHost));
	return pair_status(ctx, first_err);
}

// ---- what the matrix-core drivers of msc_score_multi and msc_search_pairs (msc_api_pairs.hip) both compute
uint64_t block_hot_size(const msc_hist_set* qset, const uint32_t* q_slots, uint64_t nq) {
	uint64_t n_hot = 0;
	for (uint64_t q = 0; q < nq; q++) n_hot += std::min(qset->mb_n_host[q_slots[q]], qset->mb_pitch);
	return n_hot;
}

// the product array of a chunk, [slices][chunk][rows] int32, is kept to 2 GiB (and the chunk to `limit` candidates)
MscCandChunks matrix_chunks(const msc_ctx* ctx, uint64_t nbins, uint64_t m, uint32_t rows, uint64_t limit) {
	const uint64_t cap = (2048ull << 20) / ((uint64_t)msc_pair_gemm_slices(nbins, (uint32_t)std::min<uint64_t>(m, 1u << 30), rows, ctx->num_cus) * rows * sizeof(int32_t));
	return msc_cand_chunks(m, std::min(cap, limit));
}

// (a folded block passes the TRUE bin count -- its transposed planes are the true ones -- and the larger of the two slice counts: room for either form)
int ensure_side(msc_ctx* ctx, BlockPipe::Side& s, uint64_t nbins, uint32_t rows, uint32_t slices, uint64_t chunk, uint64_t n_hot, HotList* hot) {
	const uint64_t nsteps = nbins / 128;
	int r;
	if ((r = ensure(ctx, s.anib, msc_pair_gemm_anib_bytes(nbins, rows))) || (r = ensure(ctx, s.qT, msc_pair_gemm_qt_bytes(nbins, rows))) ||
	    (r = ensure(ctx, s.min, (size_t)slices * chunk * rows * sizeof(int32_t))))
		return r;
	*hot = HotList();
	if (!n_hot) return MSC_OK;
	if ((r = ensure(ctx, s.hot, n_hot * 8)) || (r = ensure(ctx, s.hot_idx, 3 * (nsteps + 1) * sizeof(uint32_t))) || (r = ensure(ctx, s.diff, chunk * rows * sizeof(int32_t)))) return r;
	hot->ptr = (uint32_t*)s.hot_idx.p;
	hot->cursor = hot->ptr + (nsteps + 1);
	hot->cnt = hot->cursor + (nsteps + 1);
	return MSC_OK;
}

void fill_matrix_args(MscEpilogueArgs& ea, const BlockPipe::Side& s, const msc_hist_set* cands, const msc_hist_set* qset, uint32_t slices, uint32_t rows, uint64_t first, uint64_t n_hot, const void* emd_out) {
	ea.kb_min = (const int32_t*)s.min.p;
	ea.kb_diff = n_hot ? (const int32_t*)s.diff.p : nullptr;
	ea.kb_slices = slices; ea.kb_qn = rows; ea.kb_first = first;
	ea.kb_c_mb = cands->mb; ea.kb_c_mb_n = cands->mb_n; ea.kb_c_pitch = cands->mb_pitch;
	ea.kb_q_mb = qset->mb; ea.kb_q_mb_n = qset->mb_n; ea.kb_q_pitch = qset->mb_pitch;
	ea.kb_qT = (const uint8_t*)s.qT.p;
	ea.emd_stride = rows; ea.emd_ranks = (const uint64_t*)emd_out;
}

hipError_t launch_emd_ranks(hipStream_t st, const msc_hist_set* cands, const msc_hist_set* qset, const uint32_t* d_slots, uint64_t off, uint32_t mc, const uint32_t* dq, uint32_t nq, uint64_t* out, uint32_t stride, const uint32_t* run_if) {
	const uint64_t nbins = cands->L.nbins;
	if (cands->ranks16 && qset->ranks16 && cands->rk_pitch == qset->rk_pitch)          // every reduced rank of both sets fits 16 bits: two per v_sad_u16
		return msc_launch_emd_ranks16(st, nbins, cands->ranks16, cands->rk_pitch, cands->rk_n, d_slots, off, mc, qset->ranks16, qset->rk_n, dq, nq, out, stride, run_if);
	return msc_launch_emd_ranks(st, nbins, cands->ranks, cands->rk_pitch, cands->rk_n, d_slots, off, mc, qset->ranks, qset->rk_pitch, qset->rk_n, dq, nq, out, stride, run_if);
}

void fill_pair_args(MscEpilogueArgs& ea, msc_ctx* ctx, const msc_hist_set* cands, const msc_hist_set* qset, const uint32_t* d_slots, uint64_t first, uint32_t mc, const uint32_t* dq, uint32_t q_slot0, uint32_t nq, uint32_t n_rec, int order) {
	memset(&ea, 0, sizeof ea);
	ea.S = n_rec; ea.m = nq * mc; ea.n_queries = nq; ea.m_per_query = mc;
	ea.cand_scalars = cands->scalars + first * cands->scalar_stride; ea.cand_scalar_stride = cands->scalar_stride; ea.cand_slots = d_slots;
	ea.q_slots = dq; ea.qset_scalars = qset->scalars; ea.q_scalar_stride = qset->scalar_stride;
	ea.q_scalars = qset->scalars + (uint64_t)q_slot0 * qset->scalar_stride;
	ea.nbins = cands->L.nbins; ea.dtype = cands->dtype; ea.order = order;
	ea.error_word = (int32_t*)ctx->err_word.p;
}

void name_matrix_kernel(msc_ctx* ctx, uint32_t rows, bool emd, bool cells, bool from_lists, uint32_t fold) {
	char folded[24] = "";
	if (fold) snprintf(folded, sizeof folded, ", folded x %u", fold);
	snprintf(ctx->last_kernel_buf, sizeof ctx->last_kernel_buf, "%s<%u query rows, one matrix product per tile of presence bits%s%s%s%s>", msc_pair_gemm_kernel_name(), rows,
	         emd ? ", emd by ranks" : ", no emd", cells ? ", divergence sums from cells" : "", from_lists ? ", mirrors from lists" : "", folded);
	ctx->last_kernel = ctx->last_kernel_buf;
}

namespace {

// ---- msc_score_multi: the call, its blocks, a route per block
// ctx->open_words: {count, overflow} of a block's list of open pairs, then the call's three totals (pairs walked, blocks that overflowed, folded blocks
// that fell back), then the two words of the integer cut (msc_fold_reject.h): {pairs evaluated in rows with a cut, rows without a cut}
constexpr size_t kOpenWordsBytes = 2 * sizeof(uint32_t) + 5 * sizeof(uint64_t);
constexpr size_t kRejectWordsAt = 2 * sizeof(uint32_t) + 3 * sizeof(uint64_t);
enum Route { R_MATRIX, R_DIGEST, R_RING, R_TILES, R_SPARSE_QUEUED, R_PER_QUERY };

// what pick_route decides for one block
struct BlockRoute {
	Route kind = R_PER_QUERY;
	bool queued = false;          // matrix: the block is queued behind the one before it, and nothing waits for the stream
	uint64_t n_hot = 0;           // matrix: entries of the queries' hot list
	bool emd_ranks = false;       // matrix, digest: the earth mover's distance comes from the ranks mirrors
	int tq = 0, tps = 1;          // ring, tiles: queries per group; digest: tiles per step
	bool prefix16 = false;        // ring: 16-bit prefix form
};

struct MultiCall {
	msc_ctx* ctx;          // the arguments of msc_score_multi
	const msc_model* model;
	const msc_hist_set* cands; const uint32_t* cand_slots; uint64_t m;
	const msc_hist_set* qset; const uint32_t* q_slots; uint64_t n_q;
	int order;
	double *sum_out, *csum_out; uint8_t* close_out; uint64_t feat_mask; double* raw_out;
	uint64_t want = 0;            // the statistics of the model's singles and of feat_mask; nf: those of feat_mask, per pair of raw_out
	bool need_emd = false, want_div = false, want_grp = false;
	int nf = 0;
	const msc_hist_set *c_sp = nullptr, *q_sp = nullptr;          // sparse mirrors of dense sets, for the divergence / group passes
	bool cells = false;           // msc_set_multi_div_cells: the matrix-core blocks take the divergence sums from cells, no merge pass
	bool mirrors_settled = false; // c_sp / q_sp, grp_dense and simple are what the older routes need (with cells: not before a block falls back)
	bool grp_dense = false;       // the group passes read the dense slots
	bool kb_fit = false;          // the matrix cores can take the call's blocks
	bool reject = false;          // msc_set_fold_reject: the call's folded blocks may cut their rows (flags only, a model with an f32 image, every candidate slot holds a histogram)
	bool simple = false;          // dense sets: a block of two or more runs on one of the Q x M kernels
	uint64_t mc_ = 0, ms_ = 0;    // largest count / sum of either set
	bool compact = false, excess16 = false;
	bool queue_up = false;        // the call's query slots are in qslots_all
	bool in_flight = false;       // queued blocks have not been waited for; they share the error word, cleared by the first of them
	bool cands_up = false;        // the candidate slot list is in ctx->slots
	float ms = 0.f;               // msc_last_kernel_ms / _launches cover the whole call
	int launches = 0;
	std::vector<MscMultiBlock> blocks;
	std::vector<BlockRoute> taken;          // the routes of the blocks the matrix cores take, in the order of `blocks`
	// msc_set_query_groups: the groups of two blocks and more (msc_query_groups), the arena each was built in (-1: not yet), and per block of the plan
	// its group (-1: the block builds its own queries' side)
	std::vector<MscQueryGroup> groups;
	std::vector<int> group_arena, group_of;
	// msc_set_tail_groups: the tail groups of two blocks and more (msc_tail_groups), the side of the pipe each took (-1: not yet), and per block of the plan
	// its tail group (-1: the block runs its own tail)
	std::vector<MscTailGroup> tgroups;
	std::vector<int> tgroup_side, tgroup_of;
};

// one block of the call: its queries, its rows of the caller's arrays, and what its route's steps hand one another while it runs
struct Block {
	uint64_t q0, nq;
	const uint32_t* q_slots;
	double *sum, *csum, *raw;
	uint8_t* close;
	const uint32_t* dq_slots = nullptr;          // the query slots on the device
	uint64_t chunk = 0;                          // candidates per launch
	hipStream_t tail = nullptr;                  // where the epilogue and the copies home run
	bool div_pass = false;                       // divergence statistics from a merge pass per query (not from cells)
	uint32_t idx = 0;                            // the block's place in the call's plan
	SparseKernel spk = SPK_MP;                   // ... one merge kernel for the whole block ...
	uint32_t dvn = 1;                            // ... and its {jd, js} records per pair
};
// candidates [off, off + mc) of a block: their device slot list (or null), bins and scalars
struct Chunk { uint64_t off; uint32_t mc; const uint32_t* d_slots; const uint8_t *c_bins, *c_scal; };

// timing events of queued blocks (two per launch of the streaming kernel), kept for the life of the context
int pool_event(msc_ctx* ctx, hipEvent_t* e) {
	BlockPipe& pipe = ctx->pipe;
	if (pipe.ev_used == pipe.ev_pool.size()) {
		hipEvent_t n = nullptr;
		HIP_TRY(ctx, hipEventCreate(&n));
		pipe.ev_pool.push_back(n);
	}
	*e = pipe.ev_pool[pipe.ev_used++];
	return MSC_OK;
}

// the queued blocks: wait for them, add up their kernel times, read the error word they share
int flush_deferred(MultiCall& c) {
	if (!c.in_flight) return MSC_OK;
	c.in_flight = false;
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	hipError_t e = hipStreamSynchronize(ctx->stream);
	if (pipe.tail_used) {          // (the epilogues of the queued blocks run on the second stream)
		const hipError_t e2 = hipStreamSynchronize(pipe.tail_stream);
		if (e == hipSuccess) e = e2;
		pipe.tail_used = false;
		for (BlockPipe::Side& s : pipe.side) s.tail_busy = s.product_busy = false;          // (every product waited for its queries' side: the prep stream is idle too)
		for (BlockPipe::GroupSide& s : pipe.gside) s.tail_busy = s.product_busy = false;
	}
	for (BlockPipe::Arena& a : pipe.arena) a.busy = false;          // (what read them is through; a group built ahead of its blocks stays as it is)
	for (size_t i = 0; i + 1 < pipe.ev_used; i += 2) {
		float t = 0;
		if (e == hipSuccess && hipEventElapsedTime(&t, pipe.ev_pool[i], pipe.ev_pool[i + 1]) == hipSuccess) { c.ms += t; ctx->have_timing = true; }
	}
	pipe.ev_used = 0;
	if (e != hipSuccess) return fail(ctx, MSC_ERR_HIP, "queued blocks failed: %s", hipGetErrorString(e));
	return read_error_word(ctx);
}

// The route of block [q_slots, q_slots + nq) -- the only reader of the MSC_MULTI_*, MSC_GEMM_NO_QUEUE, MSC_SPARSE_NO_* and MSC_DIGEST_* switches
// (a route's own switches are read where its facts are gathered: matrix_facts reads MSC_NO_SCREEN and MSC_GEMM_NO_PREP, run_sparse_queued
// MSC_NO_RANKS_1XM; msc_mirrors.hip reads MSC_MULTI_NO_GEMM / _NO_RANKS and MSC_NO_RANKS16 for the mirrors).
// may_matrix: the plan offers the block to the matrix cores and only asks whether they take it; otherwise the choice is among the other routes.
//   matrix  EVERYTHING on the matrix cores (msc_pair_gemm.hip): one int8 product per tile of bins over the presence-bit mirrors + corrections from
//           the lists of large bins -- exact for any counts of the narrow range. The queries' large bins become the block's hot list (its size is
//           known here: the lists' lengths are mirrored on the host); a block whose list would average more than 64 entries per 128-bin step is
//           left to the older routes, as is one without ranks mirrors when the earth mover's distance is wanted.
//   digest  (pair_digest.hip) counts and excess prefixes within 16 bits, from four queries up: the mirror streams 4 bytes per bin, which against 8/16-bit
//           raw bins pays once enough queries share each candidate read (measured crossovers at k = 9: 7 queries for uint8_t, 5-6 for uint16_t, 4 for uint32_t)
//   ring    LDS-DMA ring over the raw bins: 32/64-bit bins, compact totals, query groups of four or eight; tiles: the raw register kernel, for everything else
//   sparse-queued  two sparse sets: a merge-path or rank-list pass per query, queued into one record array with one epilogue
//   per-query      one 1 x M pass per query (run_score): padded tiny histograms, wide sets, a single query, an unavailable sparse mirror
BlockRoute pick_route(const MultiCall& c, const uint32_t* q_slots, uint64_t nq, bool may_matrix, int* err) {
	static const bool no_digest = getenv("MSC_MULTI_NO_DIGEST") != nullptr;
	static const bool no_queue = getenv("MSC_GEMM_NO_QUEUE") != nullptr;
	static const bool no_sp_multi = getenv("MSC_SPARSE_NO_MULTI") != nullptr;
	static const bool no_ranks = getenv("MSC_MULTI_NO_RANKS") != nullptr;
	static const bool no_ring = getenv("MSC_MULTI_NO_RING") != nullptr;
	static const bool no_p16 = getenv("MSC_RING_NO_P16") != nullptr;
	const char* env_tq = getenv("MSC_MULTI_TQ");
	const bool tuned_by_hand = env_tq || getenv("MSC_DIGEST_SLOTS");          // A/B switches of the older kernels: keep to them
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	const MscLayout& L = cands->L;
	BlockRoute rt;
	*err = MSC_OK;
	if (may_matrix) {          // R_MATRIX, or any other answer: the plan then cuts the block for the older routes and asks again, block by block
		if (tuned_by_hand || no_digest || !(cands->sparse || c.simple)) return rt;
		rt.n_hot = block_hot_size(qset, q_slots, nq);
		if (rt.n_hot > 64 * (L.nbins / 128)) return rt;
		if (c.need_emd) {
			if ((*err = ensure_ranks(ctx, cands)) || (*err = ensure_ranks(ctx, qset)) || !cands->ranks || !qset->ranks) return rt;
			rt.emd_ranks = true;
		}
		rt.kind = R_MATRIX;
		rt.queued = c.n_q > 128 && !no_queue;          // (a call of one block has nothing to queue behind)
		return rt;
	}
	if (cands->sparse) {
		const bool queued = !no_sp_multi && !(c.want & (MSC_FEAT_DIV | MSC_FEAT_GROUPS)) && nq > 1 && !needs_wide(cands, qset) && c.mc_ < 65536 && nq * c.m <= 0x7fffffffull &&
		                    nq * c.m * sizeof(MscPartial) <= (4096ull << 20) && !getenv("MSC_SPARSE_NO_MP") && !getenv("MSC_SPARSE_LDS");
		rt.kind = queued ? R_SPARSE_QUEUED : R_PER_QUERY;
		return rt;
	}
	if (!c.simple || nq < 2) return rt;
	rt.tq = nq >= 4 ? 4 : 2;                     // TQ = 4 keeps the 32-bit register kernel HBM-bound
	if (env_tq) { const int v = atoi(env_tq); if (v == 2 || v == 4 || v == 8) rt.tq = v; }
	if (rt.tq > (int)nq) rt.tq = nq >= 4 ? 4 : 2;
	const uint64_t dg_min_q = cands->dtype == 8 ? 8 : cands->dtype == 16 ? 6 : 4;
	// (one digest tile per lane-run of 16 bins: wave totals of 1024 * max^2 must fit 32 bits)
	bool digest = !no_digest && c.excess16 && msc_digest_supported(L) && c.mc_ < 2048 && nq >= dg_min_q && !env_tq;
	if (digest) {
		if ((*err = ensure_digest(ctx, cands)) || (*err = ensure_digest(ctx, qset))) return rt;
		digest = cands->digest && qset->digest;
	}
	if (digest) {
		rt.kind = R_DIGEST;
		rt.tps = msc_digest_tiles_per_step(L, c.mc_);
		// The earth mover's distance from sorted k-mer ranks (msc_emd_ranks.hip) -- O(k-mers) per pair instead of O(bins): while the longest
		// list is a quarter of the bins or less, for up to 256 queries and 2^20 bins (32-bit wave sums). The digest kernel then runs its
		// count-only form (two tiles per step)
		const bool ranks_fit = !no_ranks && !tuned_by_hand && nq <= 256 && L.nbins <= (1ull << 20) && c.ms_ >= L.nbins && (c.ms_ - L.nbins) * 4 <= L.nbins;
		if (c.need_emd && ranks_fit && rt.tps == 2) {
			if ((*err = ensure_ranks(ctx, cands)) || (*err = ensure_ranks(ctx, qset))) return rt;
			rt.emd_ranks = cands->ranks && qset->ranks;
		}
		return rt;
	}
	const bool wide_bins = cands->dtype == 32 || cands->dtype == 64;
	if (nq >= 16 && !env_tq && wide_bins) rt.tq = 8;      // measured best from 16 queries up
	const bool ring = !no_ring && c.compact && L.LPT == 4 && wide_bins && (rt.tq == 4 || rt.tq == 8) && nq >= 4;
	rt.kind = ring ? R_RING : R_TILES;
	rt.prefix16 = ring && !no_p16 && c.excess16;
	return rt;
}

int begin_block(msc_ctx* ctx) {
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	ctx->tiles_ms_accum = 0.f; ctx->tiles_launches = 0; ctx->have_timing = false;
	return MSC_OK;
}

// one streaming pass per query through the single-query kernel; msc_last_close_counts keeps no counts for the call
int run_per_query(MultiCall& c, Block& b) {
	msc_ctx* ctx = c.ctx;
	ctx->close_counts_n = 0;
	float ms = 0.f;
	int launches = 0, r;
	for (uint64_t q = 0; q < b.nq; q++) {
		ScoreRequest rq;
		rq.model = c.model; rq.cands = c.cands; rq.cand_slots = c.cand_slots; rq.m = c.m; rq.qset = c.qset; rq.q_slot = b.q_slots[q]; rq.order = c.order;
		rq.feat_mask = c.feat_mask; rq.raw_out = b.raw ? b.raw + q * c.m * c.nf : nullptr; rq.sum_out = b.sum ? b.sum + q * c.m : nullptr;
		rq.csum_out = b.csum ? b.csum + q * c.m : nullptr; rq.flags_out = b.close ? b.close + q * c.m : nullptr;
		if ((r = run_score(ctx, rq))) return r;
		ms += ctx->tiles_ms_accum; launches += ctx->tiles_launches;
	}
	ctx->tiles_ms_accum = ms; ctx->tiles_launches = launches;
	return MSC_OK;
}

// the fields of the epilogue's arguments every Q x M route fills alike
void fill_block_args(const MultiCall& c, Block& b, const uint32_t* dq_slots, const Chunk& k, uint32_t n_rec, MscEpilogueArgs& ea) {
	msc_ctx* ctx = c.ctx;
	fill_pair_args(ea, ctx, c.cands, c.qset, k.d_slots, c.cand_slots ? 0 : k.off, k.mc, dq_slots, b.q_slots[0], (uint32_t)b.nq, n_rec, c.order);
	ea.partials = (const MscPartial*)ctx->partials.p;
	ea.feat_mask = c.feat_mask;
	ea.model = c.model ? c.model->d : nullptr;
	ea.raw_out = b.raw ? (double*)ctx->raw.p : nullptr;
	ea.sum_soa = b.sum ? (double*)ctx->soa_sum.p : nullptr;
	ea.csum_soa = b.csum ? (double*)ctx->soa_csum.p : nullptr;
}

// ---- the Q x M kernels over two dense sets (and the matrix cores over two sparse ones): the steps their routes share
// The block's query slots, the cleared error word and the candidate slot list, on the context's stream. A QUEUED block's query slots are part of the list the
// call sent up once, the error word is cleared by the first queued block and read after the last, the candidate list goes up once -- and nothing waits for the
// stream: the scratch buffers the next block overwrites are ordered behind this block's kernels by the stream (a buffer that has to grow goes through hipFree, which waits).
int block_uploads(MultiCall& c, Block& b, bool queued) {
	msc_ctx* ctx = c.ctx;
	int r;
	if ((r = ensure(ctx, ctx->err_word, sizeof(int32_t)))) return r;
	if (queued) b.dq_slots = (const uint32_t*)ctx->qslots_all.p + b.q0;
	else {
		if ((r = ensure(ctx, ctx->qslots, b.nq * sizeof(uint32_t)))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->qslots.p, b.q_slots, b.nq * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		b.dq_slots = (const uint32_t*)ctx->qslots.p;
	}
	if (!queued || !c.in_flight) HIP_TRY(ctx, hipMemsetAsync(ctx->err_word.p, 0, sizeof(int32_t), ctx->stream));
	if (c.cand_slots && !(queued && c.cands_up)) {
		if ((r = ensure(ctx, ctx->slots, c.m * sizeof(uint32_t)))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->slots.p, c.cand_slots, c.m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		if (queued) c.cands_up = true;
	}
	if (queued) c.in_flight = true;
	return MSC_OK;
}

// [n_q][chunk][16][2] group records are kept to 1 GiB
uint64_t group_chunk_limit(const MultiCall& c, uint64_t nq) { return c.want_grp ? (1024ull << 20) / (nq * 32 * sizeof(double)) : ~0ull; }

// Scratch of a block's chunks: the results, and what the divergence / group passes behind the streaming kernel write. Divergence statistics: the integer
// reductions come from the streaming kernel, the two FP64 sums from one merge pass per query over the sparse mirrors, queued behind it -- the
// same kernel, hence the same values, as a 1 x M pass per query. sim_mm / rre_k_r likewise: one group pass per query, over the mirrors' lists or (histograms
// under 64 KiB) the dense slots -- the kernels and records of the 1 x M pass.
int ensure_block_scratch(MultiCall& c, Block& b, bool flags_by_copy_stream) {
	msc_ctx* ctx = c.ctx;
	const uint64_t n_q = b.nq, chunk = b.chunk;
	int r;
	if (c.want_grp) {
		if ((r = ensure(ctx, ctx->grp_pairs, n_q * chunk * 32 * sizeof(double))) || (r = ensure(ctx, ctx->grp_self, (chunk + n_q) * 16 * sizeof(double)))) return r;      // [candidates][16] then [queries][16]
	}
	if (b.div_pass) {          // one kernel for the whole block: merge-path unless some query's lists are out of its range
		uint64_t q_nnz_max = 0;
		for (uint64_t q = 0; q < n_q; q++) {
			if (pick_sparse_kernel(c.c_sp, c.q_sp, b.q_slots[q], c.mc_, false) != SPK_MP) b.spk = SPK_GENERIC;
			q_nnz_max = std::max<uint64_t>(q_nnz_max, c.q_sp->hdr_host[b.q_slots[q]].nnz);
		}
		b.dvn = div_records(b.spk, q_nnz_max + c.c_sp->max_nnz);
		if ((r = ensure(ctx, ctx->div_tables, chunk * 256 * 16)) || (r = ensure(ctx, ctx->div_partials, n_q * chunk * b.dvn * 16)) ||
		    (r = ensure(ctx, ctx->sp_partials, chunk * sparse_records(b.spk) * sizeof(MscPartial))))
			return r;
	}
	if (b.sum && (r = ensure(ctx, ctx->soa_sum, n_q * chunk * sizeof(double)))) return r;
	if (b.csum && (r = ensure(ctx, ctx->soa_csum, n_q * chunk * sizeof(double)))) return r;
	if (b.close && !flags_by_copy_stream && (r = ensure(ctx, ctx->soa_close, n_q * chunk))) return r;
	if (b.close && flags_by_copy_stream && ((r = ensure(ctx, ctx->pipe.close_pp[0], n_q * chunk)) || (r = ensure(ctx, ctx->pipe.close_pp[1], n_q * chunk)))) return r;
	if (b.raw && (r = ensure(ctx, ctx->raw, n_q * chunk * c.nf * sizeof(double)))) return r;
	return MSC_OK;
}

Chunk chunk_at(const MultiCall& c, const Block& b, uint64_t off) {
	const msc_hist_set* cands = c.cands;
	const uint64_t first = c.cand_slots ? 0 : off;          // (a sparse set on the matrix-core pass has no bins, and nothing of that pass reads one)
	return Chunk{off, (uint32_t)std::min(b.chunk, c.m - off), c.cand_slots ? (const uint32_t*)c.ctx->slots.p + off : nullptr,
	             cands->bins ? cands->bins + first * cands->L.slot_bytes : nullptr, cands->scalars + first * cands->scalar_stride};
}

// the divergence and group passes of a chunk, on the context's stream behind the streaming kernel, and their part of the epilogue's arguments
int side_passes(MultiCall& c, Block& b, const Chunk& k, MscEpilogueArgs& ea) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset, *c_sp = c.c_sp, *q_sp = c.q_sp;
	const MscLayout& L = cands->L;
	const uint64_t n_q = b.nq, mc = k.mc;
	if (b.div_pass) {
		for (uint64_t q = 0; q < n_q; q++)
			HIP_TRY(ctx, launch_sparse_pass(ctx, b.spk, c_sp, cands->scalars, cands->scalar_stride, k.d_slots, k.off, mc, q_sp, b.q_slots[q],
			                                qset->scalars + (uint64_t)b.q_slots[q] * qset->scalar_stride, L.nbins, 0, 0, ~0ull, (MscPartial*)ctx->sp_partials.p,
			                                ctx->div_tables.p, (double*)ctx->div_partials.p + q * mc * b.dvn * 2, c.order, 1, b.dvn));
		ea.div_direct = (const double*)ctx->div_partials.p; ea.div_direct_n = b.dvn; ea.div_base = L.nbins;
	}
	if (c.want_grp) {
		double *gp = (double*)ctx->grp_pairs.p, *gs_c = (double*)ctx->grp_self.p, *gs_q = gs_c + b.chunk * 16;
		if (c.grp_dense) {
			HIP_TRY(ctx, msc_launch_self_markov_dense(ctx->stream, L, cands->dtype, cands->bins, k.d_slots, k.off, mc, gs_c));
			HIP_TRY(ctx, msc_launch_self_markov_dense(ctx->stream, qset->L, qset->dtype, qset->bins, b.dq_slots, 0, (uint32_t)n_q, gs_q));
			for (uint64_t q = 0; q < n_q; q++)
				HIP_TRY(ctx, msc_launch_pair_groups_dense(ctx->stream, L, cands->dtype, k.c_bins, k.c_scal, cands->scalar_stride, k.d_slots, mc,
				                                          qset->bins + (uint64_t)b.q_slots[q] * qset->L.slot_bytes, 0, 0, ~0ull, gp + q * mc * 32));
		} else {
			HIP_TRY(ctx, msc_launch_sparse_self_markov(ctx->stream, c_sp->ent, c_sp->hdr, k.d_slots, k.off, mc, gs_c));
			HIP_TRY(ctx, msc_launch_sparse_self_markov(ctx->stream, q_sp->ent, q_sp->hdr, b.dq_slots, 0, (uint32_t)n_q, gs_q));
			for (uint64_t q = 0; q < n_q; q++)
				HIP_TRY(ctx, msc_launch_pair_sparse_groups(ctx->stream, c_sp->ent, c_sp->hdr + (k.d_slots ? 0 : k.off), k.c_scal, cands->scalar_stride, k.d_slots, mc, q_sp->ent,
				                                           q_sp->hdr + b.q_slots[q], 0, 0, ~0ull, gp + q * mc * 32));
		}
		ea.grp_pairs = gp; ea.grp_self_c = gs_c; ea.grp_self_q = gs_q;
	}
	return MSC_OK;
}

// query-major [n_q][mc] on the device -> [n_q][m] at a column of the host's rows. (One chunk: the rows are contiguous on both sides -- a plain copy. A 2-D
// copy whose width is not a multiple of four bytes goes row by row inside the runtime: 1 024 rows of 6 250 flags took 9 ms of a 1.7 ms step)
hipError_t rows_home(void* dst, size_t dpitch, const void* src, size_t width, size_t rows, hipStream_t st) {
	if (dpitch == width) return hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToHost, st);
	return hipMemcpy2DAsync(dst, dpitch, src, width, width, rows, hipMemcpyDeviceToHost, st);
}

// sums and raw statistics of a chunk to the caller's arrays (the close flags go their route's own way)
int results_home(MultiCall& c, Block& b, const Chunk& k) {
	msc_ctx* ctx = c.ctx;
	const uint64_t m = c.m;
	if (b.sum) HIP_TRY(ctx, rows_home(b.sum + k.off, m * sizeof(double), ctx->soa_sum.p, (size_t)k.mc * sizeof(double), b.nq, b.tail));
	if (b.csum) HIP_TRY(ctx, rows_home(b.csum + k.off, m * sizeof(double), ctx->soa_csum.p, (size_t)k.mc * sizeof(double), b.nq, b.tail));
	if (b.raw) HIP_TRY(ctx, rows_home(b.raw + k.off * c.nf, m * c.nf * sizeof(double), ctx->raw.p, (size_t)k.mc * c.nf * sizeof(double), b.nq, b.tail));
	return MSC_OK;
}

// a chunk that is not queued is waited for, and its streaming kernel's time read
int chunk_done(msc_ctx* ctx, hipEvent_t ev_t0, hipEvent_t ev_t1) {
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	float t = 0;
	if (ctx->timing && hipEventElapsedTime(&t, ev_t0, ev_t1) == hipSuccess) { ctx->tiles_ms_accum += t; ctx->tiles_launches++; ctx->have_timing = true; }
	return MSC_OK;
}

// Sparse sets: one merge-path pass per query (up to k = 9 over the candidates' rank lists, msc_ranks_pass.hip, as in run_score), queued back
// to back into one [n_q][m] record array with ONE epilogue and one copy back -- no host round trip between the passes.
int run_sparse_queued(MultiCall& c, Block& b) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	const MscLayout& L = cands->L;
	const uint64_t n_q = b.nq, m = c.m;
	const uint32_t* q_slots = b.q_slots;
	int r;
	if ((r = begin_block(ctx))) return r;
	// (msc_launch_pair_sparse_mp hands a pass whose lists fit LDS whole to k_pair_sparse_wl: the name says which of the two the
	// queries' passes ran, "k_pair_sparse_mp+wl" when some queries fit and some do not)
	uint64_t n_wl = 0;
	for (uint64_t q = 0; q < n_q; q++) n_wl += msc_sparse_wl_fits(qset->hdr_host[q_slots[q]].nnz, cands->max_nnz) ? 1 : 0;
	ctx->last_kernel = n_wl == n_q ? "k_pair_sparse_wl" : n_wl ? "k_pair_sparse_mp+wl" : "k_pair_sparse_mp";
	ctx->last_query_tile = 1; ctx->last_partial_stride = 1;
	b.chunk = m;          // (every candidate in one launch per query: pick_route keeps n_q x m records within 4 GiB)
	b.tail = ctx->stream;
	b.div_pass = c.want_div;
	if ((r = ensure(ctx, ctx->partials, n_q * m * sizeof(MscPartial))) || (r = ensure_block_scratch(c, b, false)) || (r = block_uploads(c, b, false))) return r;
	const Chunk k = chunk_at(c, b, 0);
	const uint64_t q_kmers = qset->max_sum >= L.nbins ? qset->max_sum - L.nbins : ~0ull;
	bool rank_pass = false;
	if (getenv("MSC_NO_RANKS_1XM") == nullptr && q_kmers <= msc_ranks_pass_query_cap() && msc_ranks_pass_lds(L.nbins, q_kmers) != 0) {
		int e = MSC_OK;
		rank_pass = rank_lists_ready(ctx, cands, &e);
		if (e) return e;
		if (rank_pass && !ctx->rk_guard) {
			HIP_TRY(ctx, hipHostMalloc((void**)&ctx->rk_guard, 64, hipHostMallocDefault));
			*ctx->rk_guard = 0;
		}
		if (rank_pass && msc_ranks_pass_query_scratch(q_kmers) && (r = ensure(ctx, ctx->rk_q, msc_ranks_pass_query_scratch(q_kmers) * sizeof(uint32_t)))) return r;
		if (rank_pass) ctx->last_kernel = "k_pair_ranks_1xm";
	}
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all0, ctx->stream));
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles0, ctx->stream));
	for (uint64_t q = 0; q < n_q && rank_pass; q++)
		HIP_TRY(ctx, msc_launch_pair_ranks_1xm(ctx->stream, cands->rkl, cands->rkl_off, cands->rkl_n, cands->scalars, cands->scalar_stride, k.d_slots, 0, (uint32_t)m, qset->ent, qset->cum,
		                                       qset->hdr + q_slots[q], L.nbins, 0, 0, ~0ull, (MscPartial*)ctx->partials.p + q * m, ctx->num_cus, q_kmers, ctx->rk_guard, (uint32_t*)ctx->rk_q.p));
	for (uint64_t q = 0; q < n_q && !rank_pass; q++)
		HIP_TRY(ctx, msc_launch_pair_sparse_mp(ctx->stream, cands->ent, cands->cum, cands->hdr, cands->scalars, cands->scalar_stride, k.d_slots, (uint32_t)m, qset->ent,
		                                       qset->cum, qset->hdr + q_slots[q], qset->scalars + (uint64_t)q_slots[q] * qset->scalar_stride, L.nbins, 0, 0, ~0ull,
		                                       (MscPartial*)ctx->partials.p + q * m, nullptr, nullptr, c.order, ctx->num_cus,
		                                       (uint32_t)std::min<uint64_t>(0x7fffffffull, (uint64_t)qset->hdr_host[q_slots[q]].nnz + cands->max_nnz), 1,
		                                       qset->hdr_host[q_slots[q]].nnz, cands->max_nnz));
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles1, ctx->stream));
	MscEpilogueArgs ea;
	fill_block_args(c, b, b.dq_slots, k, 1, ea);
	ea.sparse_base = L.nbins;
	ea.close_soa = b.close ? (uint8_t*)ctx->soa_close.p : nullptr;
	HIP_TRY(ctx, msc_launch_epilogue(ctx->stream, ea));
	if (b.close && ctx->close_counts_n) HIP_TRY(ctx, msc_launch_close_counts(ctx->stream, (const uint8_t*)ctx->soa_close.p, (uint32_t)n_q, (uint32_t)m, (uint64_t*)ctx->close_counts.p + b.q0));
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all1, ctx->stream));
	if ((r = results_home(c, b, k))) return r;
	if (b.close) HIP_TRY(ctx, hipMemcpyAsync(b.close, ctx->soa_close.p, n_q * m, hipMemcpyDeviceToHost, ctx->stream));
	int32_t first_err = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&first_err, ctx->err_word.p, sizeof first_err, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	float t = 0;
	if (ctx->timing && hipEventElapsedTime(&t, ctx->ev_tiles0, ctx->ev_tiles1) == hipSuccess) { ctx->tiles_ms_accum = t; ctx->tiles_launches = (int)n_q; ctx->have_timing = true; }
	if (rank_pass && *ctx->rk_guard) {
		*ctx->rk_guard = 0;
		return fail(ctx, MSC_ERR_HIP, "rank pass: a query's list is longer than its set's bound (max_sum not maintained by a writer of that set)");
	}
	return pair_status(ctx, first_err);
}

// The digest, ring and raw-tile kernels: partial records per (query, candidate), folded by the epilogue; one chunk at a time, waited for.
int run_streamed(MultiCall& c, Block& b, const BlockRoute& rt) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	const MscLayout& L = cands->L;
	const uint64_t n_q = b.nq, m = c.m;
	const bool digest = rt.kind == R_DIGEST, ring = rt.kind == R_RING;
	int r;
	if ((r = begin_block(ctx))) return r;
	b.tail = ctx->stream;
	b.div_pass = c.want_div;
	if ((r = block_uploads(c, b, false))) return r;
	const bool digest_emd = c.need_emd && !rt.emd_ranks;          // the digest kernel streams and scores the prefix half
	const bool count_only = digest && rt.tps == 2 && !digest_emd;
	// the digest kernel writes one record per step of tps tiles, four groups of four queries per workgroup; partial records of one launch
	// are capped at 4 GiB: equal candidate chunks
	const uint32_t n_rec = digest ? (uint32_t)(L.nbins / 1024) / rt.tps : L.S;
	const uint64_t rec_bytes = digest || ring ? 16 : sizeof(MscPartial);
	const uint64_t q_rows = digest ? (n_q + 15) / 16 * 16 : ring ? (n_q + rt.tq - 1) / rt.tq * rt.tq : n_q;       // records cover the padded query count
	b.chunk = msc_cand_chunks(m, std::min<uint64_t>((4096ull << 20) / ((uint64_t)n_rec * rec_bytes * q_rows), group_chunk_limit(c, n_q))).chunk;
	if ((r = ensure(ctx, ctx->partials, q_rows * b.chunk * n_rec * rec_bytes)) || (r = ensure_block_scratch(c, b, false))) return r;
	if (rt.emd_ranks && (r = ensure(ctx, ctx->emd_out, b.chunk * 64 * sizeof(uint64_t)))) return r;
	if (digest) {
		snprintf(ctx->last_kernel_buf, sizeof ctx->last_kernel_buf, "k_pair_digest_multi<%s counts%s>", c.mc_ < 256 ? "u8" : "u16", rt.emd_ranks ? ", emd by ranks" : count_only ? ", no emd" : "");
		ctx->last_kernel = ctx->last_kernel_buf;
	} else ctx->last_kernel = ring ? "k_pair_tiles_multi32_ring" : "k_pair_tiles_multi";
	// the digest kernel's workgroup scores up to 16 queries per candidate tile it fetches; the ring kernel's co-located query
	// blocks fetch the tile once per group of tq queries (the followers usually hit in L2, which is not counted on)
	ctx->last_query_tile = (int)std::min<uint64_t>(n_q, digest ? 16 : (uint64_t)rt.tq);
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all0, ctx->stream));
	for (uint64_t off = 0; off < m; off += b.chunk) {
		const Chunk k = chunk_at(c, b, off);
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles0, ctx->stream));
		if (digest)
			HIP_TRY(ctx, msc_launch_pair_digest_multi(ctx->stream, L, cands->digest + (c.cand_slots ? 0 : off * msc_digest_slot_bytes(L)), k.d_slots, k.mc, qset->digest,
			                                          b.dq_slots, (uint32_t)n_q, c.mc_ < 256, rt.tps, digest_emd, ctx->partials.p, ctx->num_cus, true, 4));
		else if (ring)
			HIP_TRY(ctx, msc_launch_pair_tiles_multi_ring(ctx->stream, L, cands->dtype, k.c_bins, k.c_scal, k.d_slots, k.mc, qset->bins, qset->L.slot_bytes, qset->scalars,
			                                              qset->scalar_stride, b.dq_slots, (uint32_t)n_q, rt.tq, rt.prefix16, ctx->partials.p, ctx->num_cus));
		else
			HIP_TRY(ctx, msc_launch_pair_tiles_multi(ctx->stream, L, cands->dtype, k.c_bins, k.c_scal, k.d_slots, k.mc, qset->bins, qset->L.slot_bytes, qset->scalars,
			                                         qset->scalar_stride, b.dq_slots, (uint32_t)n_q, rt.tq, c.compact, (MscPartial*)ctx->partials.p, ctx->num_cus));
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles1, ctx->stream));
		if (rt.emd_ranks) HIP_TRY(ctx, launch_emd_ranks(ctx->stream, cands, qset, k.d_slots, off, k.mc, b.dq_slots, (uint32_t)n_q, (uint64_t*)ctx->emd_out.p, 64));
		MscEpilogueArgs ea;
		fill_block_args(c, b, b.dq_slots, k, n_rec, ea);
		if ((r = side_passes(c, b, k, ea))) return r;
		ea.partials16 = ring ? ctx->partials.p : nullptr;
		ea.partials_cq = digest ? ctx->partials.p : nullptr;
		ea.cq_group = 16;
		if (rt.emd_ranks) ea.emd_ranks = (const uint64_t*)ctx->emd_out.p;
		ea.close_soa = b.close ? (uint8_t*)ctx->soa_close.p : nullptr;
		HIP_TRY(ctx, msc_launch_epilogue(ctx->stream, ea));
		if (b.close && ctx->close_counts_n) HIP_TRY(ctx, msc_launch_close_counts(ctx->stream, ea.close_soa, (uint32_t)n_q, k.mc, (uint64_t*)ctx->close_counts.p + b.q0));
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all1, ctx->stream));
		if ((r = results_home(c, b, k))) return r;
		if (b.close) HIP_TRY(ctx, rows_home(b.close + off, m, ea.close_soa, (size_t)k.mc, n_q, ctx->stream));
		if ((r = chunk_done(ctx, ctx->ev_tiles0, ctx->ev_tiles1))) return r;
	}
	return read_error_word(ctx);
}

// The matrix cores. Queued blocks run in stages on three streams (BlockPipe, msc_objects.h): the product of block i on the context's stream beside the rank
// walk of block i and the epilogue of block i - 1 on tail_stream, the queries' side of block i + 1 on prep_stream -- the product is bound by the matrix pipe,
// the others by vector arithmetic and latency. Blocks take turns on the two sides of the pipe. (Single chunk, no divergence / group passes between the stages -- divergence sums from cells run none;
// MSC_GEMM_NO_PREP: the queries' side on the product's stream, as in r04.) The close flags go into one of two buffers and home on the copy stream, under the next block's kernels.
// A flags-only block whose distance comes from the ranks mirrors runs no walk beside the product: its tail is the bound screen, the walk and the FP64 evaluation of
// the listed pairs, then the dense walk and the two older epilogue kernels predicated on the list's overflow word (msc_emd_list.hip).
// Such a block in one chunk runs its product over bits folded F-to-1 where both sets carry the folded mirror (msc_fold.h).
// Consecutive FOLDED blocks of one such group share ONE tail too (plan_tail_groups, tail_group_slot, group_tail; msc_set_tail_groups): their products stay one launch per block,
// each into its slot of one of two group sides, and the group's last block issues every kernel behind them once, blockIdx.y the block.
// Consecutive piped blocks of 128 rows share ONE build of the queries' side (plan_query_groups, group_side; msc_set_query_groups): a group's images and lists lie in one of
// two arenas, built on the prep stream a group ahead of the blocks that read them; such a block's qT, anib and hot list are views into the arena.
// What a block decides is plain arithmetic (msc_matrix_stages, msc_multi_plan.h) over facts gathered in one place (matrix_facts); run_matrix is the order of the
// stages, one function each. A stage issues, in its own order, everything it puts on a stream: a re-cut of what was one body, in the same order.

// what a block on the matrix cores settles first: its query rows, its candidates per launch, whether a merge pass serves the divergence sums
uint32_t settle_matrix_block(const MultiCall& c, Block& b) {
	const uint32_t rows = msc_pair_gemm_rows((uint32_t)b.nq);
	b.chunk = matrix_chunks(c.ctx, c.cands->L.nbins, c.m, rows, group_chunk_limit(c, b.nq)).chunk;
	b.div_pass = c.want_div && !c.cells;
	return rows;
}

// the product arrays of a side alone (a grouped block: its images and lists are views into its group's arena)
int ensure_products(msc_ctx* ctx, BlockPipe::Side& s, uint32_t rows, uint32_t slices, uint64_t chunk, uint64_t n_hot) {
	int r;
	if ((r = ensure(ctx, s.min, (size_t)slices * chunk * rows * sizeof(int32_t)))) return r;
	return n_hot ? ensure(ctx, s.diff, chunk * rows * sizeof(int32_t)) : MSC_OK;
}

// the facts of a block on the matrix cores -- beside pick_route the only reader of environment switches here: MSC_NO_SCREEN (FP64 for every pair of
// a flags-only block), MSC_GEMM_NO_PREP. second_run: rerun_overflowed's
MscMatrixFacts matrix_facts(const MultiCall& c, const Block& b, const BlockRoute& rt, bool second_run) {
	static const bool no_screen = getenv("MSC_NO_SCREEN") != nullptr;
	static const bool no_prep = getenv("MSC_GEMM_NO_PREP") != nullptr;
	const msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	MscMatrixFacts f;
	f.model = c.model != nullptr; f.screen_ok = c.model && c.model->h.screen_ok;
	f.close = b.close != nullptr; f.sum = b.sum != nullptr; f.csum = b.csum != nullptr; f.raw = b.raw != nullptr;
	f.want_div = c.want_div; f.want_grp = c.want_grp; f.div_pass = b.div_pass;
	f.no_screen = no_screen; f.no_prep = no_prep;
	f.queued = rt.queued; f.emd_ranks = rt.emd_ranks;
	f.block_pipe = ctx->block_pipe; f.emd_bounds = ctx->emd_bounds; f.fold_screen = ctx->fold_screen;
	f.emd_decides = c.model && c.model->emd_decides; f.fold_overflows = c.model && c.model->fold_overflows;
	f.rk_pitch_c = cands->rk_pitch; f.rk_pitch_q = qset->rk_pitch; f.moments_c = cands->rk_sum != nullptr; f.moments_q = qset->rk_sum != nullptr;
	f.kbf_c = cands->kbf != nullptr; f.kbf_q = qset->kbf != nullptr; f.kbf_fold_c = cands->kbf_fold; f.kbf_fold_q = qset->kbf_fold;
	f.second_run = second_run;
	f.n_q = b.nq; f.m = c.m; f.chunk = b.chunk;
	return f;
}

Block block_of(const MultiCall& c, size_t i);

// msc_set_query_groups: the groups of the call's plan (msc_query_groups, msc_multi_plan.h) -- a block joins on the stage decisions it will take when it runs
// (its route, the call and the context's switches settle them: nothing a block before it does changes them)
constexpr uint64_t kArenaBudget = 512ull << 20;
void plan_query_groups(MultiCall& c) {
	msc_ctx* ctx = c.ctx;
	c.groups.clear(); c.group_arena.clear(); c.group_of.clear();
	if (ctx->query_groups < 2) return;
	std::vector<MscGroupBlock> gb(c.blocks.size(), MscGroupBlock{false, 0, 0});
	size_t next_taken = 0;
	for (size_t i = 0; i < c.blocks.size(); i++) {
		if (!c.blocks[i].matrix) continue;
		const BlockRoute& rt = c.taken[next_taken++];
		Block b = block_of(c, i);
		const uint32_t rows = settle_matrix_block(c, b);
		const MscMatrixStages st = msc_matrix_stages(matrix_facts(c, b, rt, false));
		gb[i] = MscGroupBlock{st.piped && rows == 128, st.fold, rt.n_hot};
	}
	std::vector<MscQueryGroup> all;
	msc_query_groups(gb, c.cands->L.nbins, ctx->query_groups, kArenaBudget, all);
	c.group_of.assign(c.blocks.size(), -1);
	for (const MscQueryGroup& g : all) {
		if (g.n < 2) continue;          // (a group of one block: the per-block path)
		for (size_t i = g.first; i < g.first + g.n; i++) c.group_of[i] = (int)c.groups.size();
		c.groups.push_back(g);
	}
	c.group_arena.assign(c.groups.size(), -1);
}

// msc_set_tail_groups: the tail groups of the call's plan (msc_tail_groups, msc_multi_plan.h), inside its query groups -- a block joins on the stage decisions
// it will take when it runs, as above. MSC_TAIL_NO_RAMP (read when the context is made) keeps full groups to the call's end.
constexpr uint64_t kTailSideBudget = 1024ull << 20;
void plan_tail_groups(MultiCall& c) {
	msc_ctx* ctx = c.ctx;
	c.tgroups.clear(); c.tgroup_side.clear(); c.tgroup_of.clear();
	if (ctx->tail_groups < 2 || c.groups.empty()) return;
	std::vector<MscTailBlock> tb(c.blocks.size(), MscTailBlock{false, -1, 0});
	size_t next_taken = 0;
	uint32_t slices_f = 0;
	for (size_t i = 0; i < c.blocks.size(); i++) {
		if (!c.blocks[i].matrix) continue;
		const BlockRoute& rt = c.taken[next_taken++];
		if (c.group_of[i] < 0) continue;
		Block b = block_of(c, i);
		const uint32_t rows = settle_matrix_block(c, b);
		const MscMatrixStages st = msc_matrix_stages(matrix_facts(c, b, rt, false));
		const bool joins = st.piped && rows == 128 && b.chunk == c.m && b.close && msc_matrix_chunk(st, b.nq, c.m).tail == MSC_TAIL_FOLDED;
		tb[i] = MscTailBlock{joins, c.group_of[i], rt.n_hot};
		if (joins && !slices_f) slices_f = msc_pair_gemm_slices(c.cands->L.nbins / st.fold, (uint32_t)b.chunk, rows, ctx->num_cus);          // (one for all: the blocks of a query group agree on the fold)
	}
	if (!slices_f) return;
	std::vector<MscTailGroup> all;
	msc_tail_groups(tb, c.m, slices_f, ctx->tail_groups, kTailSideBudget, ctx->tail_ramp, all);
	c.tgroup_of.assign(c.blocks.size(), -1);
	for (const MscTailGroup& g : all) {
		if (g.n < 2) continue;          // (a group of one block: the per-block path)
		for (size_t i = g.first; i < g.first + g.n; i++) c.tgroup_of[i] = (int)c.tgroups.size();
		c.tgroups.push_back(g);
	}
	c.tgroup_side.assign(c.tgroups.size(), -1);
}

// a block on the matrix cores: what is settled before anything of it is issued, and what its stages hand one another
struct MatrixBlock {
	MscMatrixStages st;                               // the decisions
	const BlockRoute* rt = nullptr;
	uint32_t rows = 0, slices = 0, slices_f = 0;      // query rows of the product; slices of its array over the true bins, and over the bins it runs on
	uint64_t nbins_f = 0;                             // the bins the product runs on: 4^k, folded 4^k / fold
	int pb = 0;                                       // the side of the pipe the block takes
	BlockPipe::Side* s = nullptr;
	hipStream_t prep = nullptr;                       // where the queries' side runs
	HotList hot;
	int group = -1;                                   // the block's group of the call (-1: none: the images below are its side's own)
	const uint8_t *qT = nullptr, *anib = nullptr;     // the queries' images and the entries of the hot list: the side's buffers, or views into the group's arena
	const void* hot_entries = nullptr;
	int tgroup = -1;                                  // the block's tail group of the call (-1: none: it runs its own tail, and the arrays below are its side's own)
	int32_t *out_min = nullptr, *out_diff = nullptr;  // where the product writes P1 and P2: the side's arrays, or the block's slot of its tail group's side
};
// a chunk's tail: the epilogue's arguments, and the one of the two buffers its close flags go into
struct Tail { MscEpilogueArgs ea; int pp = 0; uint8_t* d_close = nullptr; };

// (b.chunk and b.div_pass are set) -- takes the block's turn on the pipe and names its streams
MatrixBlock plan_matrix(const MultiCall& c, Block& b, const BlockRoute& rt, uint32_t rows, bool second_run) {
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	const uint64_t nbins = c.cands->L.nbins;
	MatrixBlock p;
	p.st = msc_matrix_stages(matrix_facts(c, b, rt, second_run));
	p.rt = &rt;
	p.rows = rows;
	p.slices = msc_pair_gemm_slices(nbins, (uint32_t)b.chunk, rows, ctx->num_cus);
	p.nbins_f = p.st.fold ? nbins / p.st.fold : nbins;
	p.slices_f = p.st.fold ? msc_pair_gemm_slices(p.nbins_f, (uint32_t)b.chunk, rows, ctx->num_cus) : p.slices;
	p.pb = p.st.piped ? (int)(pipe.next++ & 1) : 0;
	p.s = &pipe.side[p.pb];
	b.tail = p.st.piped ? pipe.tail_stream : ctx->stream;
	p.prep = p.st.own_prep_stream ? pipe.prep_stream : ctx->stream;
	return p;
}

// before a side is reused: a block on ONE stream after piped ones waits for every epilogue in flight; a piped one for the epilogue that read its side
int wait_side_free(msc_ctx* ctx, const MatrixBlock& p) {
	BlockPipe& pipe = ctx->pipe;
	if (!pipe.tail_used) return MSC_OK;
	for (int i = 0; i < 2; i++)
		if (pipe.side[i].tail_busy && (!p.st.piped || i == p.pb)) {
			HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, pipe.side[i].ev_tail, 0));
			if (p.prep != ctx->stream && p.group < 0) HIP_TRY(ctx, hipStreamWaitEvent(p.prep, pipe.side[i].ev_tail, 0));          // (it rewrites the transposed image that epilogue read; a grouped block's image is its arena's)
			if (!p.st.piped) pipe.side[i].tail_busy = false;
		}
	for (BlockPipe::GroupSide& g : pipe.gside)          // (the tails of the tail groups are epilogues in flight like any other)
		if (g.tail_busy && !p.st.piped) { HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, g.ev_tail, 0)); g.tail_busy = false; }
	return MSC_OK;
}

// A block of a tail group takes its slot of the group's side. The group's first block takes the side whose turn it is, has the product's stream wait -- once
// for the group -- for the tail that last read that side, and clears the P2 of all the group's blocks in one call.
int tail_group_slot(MultiCall& c, const Block& b, MatrixBlock& p) {
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	const MscTailGroup& T = c.tgroups[p.tgroup];
	int r;
	if (b.idx == T.first) {
		const int si = (int)(pipe.gside_next++ & 1);
		BlockPipe::GroupSide& g = pipe.gside[si];
		if ((r = ensure(ctx, g.buf, T.bytes))) return r;
		if (g.tail_busy) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, g.ev_tail, 0));
		if (T.diff_stride) HIP_TRY(ctx, hipMemsetAsync((uint8_t*)g.buf.p + T.diff_off, 0, T.n * T.diff_stride, ctx->stream));
		c.tgroup_side[p.tgroup] = si;
	}
	BlockPipe::GroupSide& g = pipe.gside[c.tgroup_side[p.tgroup]];
	const uint64_t j = b.idx - T.first;
	p.s = &g;
	p.out_min = (int32_t*)((uint8_t*)g.buf.p + T.min_off + j * T.min_stride);
	p.out_diff = T.diff_stride ? (int32_t*)((uint8_t*)g.buf.p + T.diff_off + j * T.diff_stride) : nullptr;
	return MSC_OK;
}

// the queries' side of the block, once for all chunks of candidates, on its stream; the product's stream waits for it (ev_prep)
int queries_side(const MultiCall& c, const Block& b, const MatrixBlock& p) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set* qset = c.qset;
	const uint64_t nbins = c.cands->L.nbins, n_hot = p.rt->n_hot;
	const uint32_t n_q = (uint32_t)b.nq, rows = p.rows;
	BlockPipe::Side& s = *p.s;
	hipStream_t prep = p.prep;
	if (prep != ctx->stream) {
		HIP_TRY(ctx, hipStreamWaitEvent(prep, ctx->pipe.ev_call, 0));          // the call's query slots are up
		if (s.product_busy) HIP_TRY(ctx, hipStreamWaitEvent(prep, s.ev_product, 0));      // the product that read this side is through
	}
	if (p.st.fold) {          // the transposed planes from the true mirror (the epilogue's walk of the candidate's large bins stays exact), the tiles and the hot list folded
		HIP_TRY(ctx, msc_launch_kb_gather(prep, nbins, qset->kb, b.dq_slots, n_q, rows, (uint8_t*)s.qT.p, nullptr));
		HIP_TRY(ctx, msc_launch_kb_gather(prep, p.nbins_f, qset->kbf, b.dq_slots, n_q, rows, nullptr, (uint8_t*)s.anib.p));
		HIP_TRY(ctx, msc_launch_hot_list(prep, nbins, p.st.fold, qset->mb, qset->mb_n, qset->mb_pitch, b.dq_slots, n_q, rows, (uint8_t*)s.qT.p, n_hot, s.hot.p, p.hot.ptr,
		                                 p.hot.cursor, p.hot.cnt));
	} else
		HIP_TRY(ctx, msc_launch_pair_gemm_queries(prep, nbins, qset->kb, qset->mb, qset->mb_n, qset->mb_pitch, b.dq_slots, n_q, rows, (uint8_t*)s.qT.p, n_hot, s.hot.p,
		                                          p.hot.ptr, p.hot.cursor, p.hot.cnt, (uint8_t*)s.anib.p));
	if (prep != ctx->stream) {
		HIP_TRY(ctx, hipEventRecord(s.ev_prep, prep));
		HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s.ev_prep, 0));
	}
	return MSC_OK;
}

// the queries' side of group g of the call, in the arena whose turn it is, on the prep stream (or the context's): once the call's query slots are up and
// the last block that read the arena is through with its product and its tail (both streams run their blocks in order: the last block's events cover the group)
int build_group_side(MultiCall& c, int g, hipStream_t prep) {
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	const msc_hist_set* qset = c.qset;
	const MscQueryGroup& G = c.groups[g];
	const int ai = (int)(pipe.arena_next++ & 1);
	BlockPipe::Arena& A = pipe.arena[ai];
	int r;
	if ((r = ensure(ctx, A.buf, G.bytes))) return r;
	if (prep != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(prep, pipe.ev_call, 0));
	if (A.busy) {
		if (prep != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(prep, A.last->ev_product, 0));
		HIP_TRY(ctx, hipStreamWaitEvent(prep, A.last->ev_tail, 0));
		A.busy = false;
	}
	uint8_t* base = (uint8_t*)A.buf.p;
	const MscMultiBlock& last = c.blocks[G.first + G.n - 1];
	HIP_TRY(ctx, msc_launch_query_group(prep, c.cands->L.nbins, G.fold, qset->kb, qset->kbf, qset->mb, qset->mb_n, qset->mb_pitch, (const uint32_t*)ctx->qslots_all.p + c.blocks[G.first].q0,
	                                    (uint32_t)G.n, (uint32_t)last.nq, base + G.qt_off, G.qt_stride, base + G.anib_off, G.anib_stride, G.hot_stride, base + G.hot_off,
	                                    (uint32_t*)(base + G.ptr_off), (uint32_t*)(base + G.cursor_off), (uint32_t*)(base + G.cnt_off), G.idx_stride));
	if (prep != ctx->stream) HIP_TRY(ctx, hipEventRecord(A.ev_ready, prep));
	c.group_arena[g] = ai;
	return MSC_OK;
}

// The queries' side of a block of a group: views into the group's arena. The group's first block sees to it that the side is built -- and, on a prep stream
// of its own, the next group's too, under this group's blocks -- and has the product's stream wait for it, once for the group.
int group_side(MultiCall& c, const Block& b, MatrixBlock& p) {
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	const int g = p.group;
	const MscQueryGroup& G = c.groups[g];
	int r;
	if (b.idx == G.first) {
		if (c.group_arena[g] < 0 && (r = build_group_side(c, g, p.prep))) return r;
		if (p.prep != ctx->stream) {
			HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, pipe.arena[c.group_arena[g]].ev_ready, 0));
			if (g + 1 < (int)c.groups.size() && (r = build_group_side(c, g + 1, p.prep))) return r;
		}
	}
	BlockPipe::Arena& A = pipe.arena[c.group_arena[g]];
	const uint64_t j = b.idx - G.first;
	uint8_t* base = (uint8_t*)A.buf.p;
	p.qT = base + G.qt_off + j * G.qt_stride;
	p.anib = base + G.anib_off + j * G.anib_stride;
	p.hot = HotList();
	if (p.rt->n_hot) {
		p.hot_entries = base + G.hot_off + j * G.hot_stride * 8;
		p.hot.ptr = (uint32_t*)(base + G.ptr_off) + j * G.idx_stride;
		p.hot.cursor = (uint32_t*)(base + G.cursor_off) + j * G.idx_stride;
		p.hot.cnt = (uint32_t*)(base + G.cnt_off) + j * G.idx_stride;
	}
	A.last = p.s; A.busy = true;          // (this block's product and tail are queued before anything asks)
	return MSC_OK;
}

// the whole pass over a chunk's bins: products and level products on the matrix cores, timed as the streaming kernel between ev_t0 and ev_t1
int product_stage(const MultiCall& c, const Block& b, const MatrixBlock& p, const Chunk& k, hipEvent_t ev_t0, hipEvent_t ev_t1) {
	msc_ctx* ctx = c.ctx;
	BlockPipe::Side& s = *p.s;
	const bool grouped = p.tgroup >= 0;          // (a tail group's tail waits for its last product, which is behind every such mark: no ev_head)
	const bool last_of_group = grouped && b.idx + 1 == c.tgroups[p.tgroup].first + c.tgroups[p.tgroup].n;
	if (p.st.piped && !grouped) {          // everything the tail needs from this stream so far (slot lists, the cleared error word) is behind this mark
		HIP_TRY(ctx, hipEventRecord(s.ev_head, ctx->stream));
		HIP_TRY(ctx, hipStreamWaitEvent(b.tail, s.ev_head, 0));
	}
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ev_t0, ctx->stream));
	HIP_TRY(ctx, msc_launch_pair_gemm(ctx->stream, p.nbins_f, p.st.fold ? c.cands->kbf : c.cands->kb, k.d_slots, k.off, k.mc, p.rows, p.slices_f, p.hot.ptr, p.hot_entries, p.out_min,
	                                  p.out_diff, p.anib, grouped));
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ev_t1, ctx->stream));
	if (p.st.piped && (!grouped || last_of_group)) { HIP_TRY(ctx, hipEventRecord(s.ev_product, ctx->stream)); s.product_busy = true; }
	return MSC_OK;
}

// What every tail does ahead of its epilogue kernels: the epilogue's arguments (the divergence / group passes with them, on the context's stream), a buffer for
// the flags once its last copy home is through, and the wait for the product. (A tail's kernels that read nothing of the product are queued BEFORE this.)
int tail_ready(MultiCall& c, Block& b, const MatrixBlock& p, const Chunk& k, Tail& t) {
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	const BlockRoute& rt = *p.rt;
	MscEpilogueArgs& ea = t.ea;
	int r;
	fill_block_args(c, b, b.dq_slots, k, c.cands->L.S, ea);
	if ((r = side_passes(c, b, k, ea))) return r;
	fill_matrix_args(ea, *p.s, c.cands, c.qset, p.slices, p.rows, c.cand_slots ? 0 : k.off, rt.n_hot, rt.emd_ranks ? ctx->emd_out.p : nullptr);
	ea.kb_qT = p.qT;
	ea.cq_group = 16;
	if (c.cells) { ea.div_cells = 1; ea.kb_c_bits = c.cands->kb; }          // the two sums in the epilogue, as msc_search_pairs sets them (msc_api_pairs.hip)
	t.pp = pipe.close_pp_next;
	t.d_close = b.close ? (uint8_t*)pipe.close_pp[t.pp].p : nullptr;
	if (b.close) {
		pipe.close_pp_next ^= 1;
		if (pipe.close_pp_busy[t.pp]) HIP_TRY(ctx, hipStreamWaitEvent(b.tail, pipe.ev_copied[t.pp], 0));
	}
	ea.close_soa = t.d_close;
	ea.screen = p.st.screen;
	if (p.st.piped) HIP_TRY(ctx, hipStreamWaitEvent(b.tail, p.s->ev_product, 0));
	return MSC_OK;
}

// the scored tail: the rank walk of every pair where the distance comes from the ranks mirrors (beside the product), then the epilogue
int tail_scored(MultiCall& c, Block& b, const MatrixBlock& p, const Chunk& k, Tail& t) {
	msc_ctx* ctx = c.ctx;
	int r;
	if (p.rt->emd_ranks) HIP_TRY(ctx, launch_emd_ranks(b.tail, c.cands, c.qset, k.d_slots, k.off, k.mc, b.dq_slots, (uint32_t)b.nq, (uint64_t*)ctx->emd_out.p, p.rows));
	if ((r = tail_ready(c, b, p, k, t))) return r;
	HIP_TRY(ctx, msc_launch_epilogue(b.tail, t.ea));
	return MSC_OK;
}

// the list of open pairs of a chunk and their distances (the list's words were allocated and cleared when the call began, on the product's stream: behind ev_head
// for a piped block)
int ensure_open_list(msc_ctx* ctx, uint32_t open_cap) {
	int r;
	if ((r = ensure(ctx, ctx->open_list, std::max<size_t>(1, open_cap) * sizeof(uint32_t))) || (r = ensure(ctx, ctx->emd_list, std::max<size_t>(1, open_cap) * sizeof(uint64_t)))) return r;
	return MSC_OK;
}

// the arguments of the bound screen: the epilogue's, with the moments and the list in place of the distances
MscEpilogueArgs bound_args(const MultiCall& c, const MscEpilogueArgs& ea, uint32_t open_cap) {
	msc_ctx* ctx = c.ctx;
	MscEpilogueArgs eb = ea;
	eb.emd_ranks = nullptr;
	eb.rk_c_sum = c.cands->rk_sum; eb.rk_c_dev = c.cands->rk_dev; eb.rk_q_sum = c.qset->rk_sum; eb.rk_q_dev = c.qset->rk_dev;
	eb.open_list = (uint32_t*)ctx->open_list.p; eb.open_words = (uint32_t*)ctx->open_words.p; eb.open_cap = open_cap; eb.emd_list = (const uint64_t*)ctx->emd_list.p;
	return eb;
}

// the list stage, on e's words: the bound screen, the walk of the listed pairs, their FP64 evaluation
int list_stage(const MultiCall& c, const Block& b, const MatrixBlock& p, const Chunk& k, const MscEpilogueArgs& e, uint32_t open_cap) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	const MscLayout& L = cands->L;
	const BlockPipe::Side& s = *p.s;
	const bool u16 = cands->ranks16 && qset->ranks16;
	HIP_TRY(ctx, msc_launch_epilogue_bound(b.tail, e));
	if (e.fold_x_c) {          // (the listed pairs of a folded stage: their exact P1 / P2 into the product's arrays first)
		const MscFoldExact fx{cands->ranks, cands->rk_pitch, L.nbins, L.E, L.R, k.d_slots, k.off, k.mc, b.dq_slots, e.open_list, e.open_words, open_cap, p.qT, p.rows,
		                      qset->mb, qset->mb_n, qset->mb_pitch, (int32_t*)s.min.p, e.kb_slices, p.rt->n_hot ? (int32_t*)s.diff.p : nullptr};
		HIP_TRY(ctx, msc_launch_fold_exact_list(b.tail, fx, ctx->num_cus));
	}
	HIP_TRY(ctx, msc_launch_emd_ranks_list(b.tail, u16, u16 ? (const void*)cands->ranks16 : (const void*)cands->ranks, u16 ? (const void*)qset->ranks16 : (const void*)qset->ranks,
	                                       cands->rk_pitch, k.d_slots, k.off, k.mc, b.dq_slots, e.open_list, e.open_words, open_cap, (uint64_t*)ctx->emd_list.p, ctx->num_cus));
	HIP_TRY(ctx, msc_launch_epilogue_list(b.tail, e, ctx->num_cus));
	return MSC_OK;
}

// the bounds tail: the list stage; then today's three kernels, which return at once unless the list overflowed (then they overwrite every flag of the chunk);
// then the list's words into the call's totals, cleared for the next block
int tail_bounds(MultiCall& c, Block& b, const MatrixBlock& p, const Chunk& k, uint32_t open_cap, Tail& t) {
	msc_ctx* ctx = c.ctx;
	uint32_t* open_words = (uint32_t*)ctx->open_words.p;
	int r;
	if ((r = ensure_open_list(ctx, open_cap)) || (r = tail_ready(c, b, p, k, t)) || (r = list_stage(c, b, p, k, bound_args(c, t.ea, open_cap), open_cap))) return r;
	HIP_TRY(ctx, launch_emd_ranks(b.tail, c.cands, c.qset, k.d_slots, k.off, k.mc, b.dq_slots, (uint32_t)b.nq, (uint64_t*)ctx->emd_out.p, p.rows, open_words + 1));
	t.ea.run_if = open_words + 1;
	HIP_TRY(ctx, msc_launch_epilogue(b.tail, t.ea));
	HIP_TRY(ctx, msc_launch_emd_list_close(b.tail, open_words, open_cap, (uint64_t*)(open_words + 2), nullptr));
	return MSC_OK;
}

// The integer cut of a folded tail's rows (msc_fold_reject.h), ahead of its screen: T for rows [q0, q0 + n_out) of the call -- those past n_rows get none --
// into ctx->reject_cut, from the queries' records, moments, collisions and lists, the ranges of the candidates' set (run_matrix has brought them up to date on the
// context's stream, ahead of the product this tail waits for) and the model. e: the screen's arguments, which take the cuts and the counter.
int cut_rows(const MultiCall& c, hipStream_t tail, const uint32_t* dq_slots, uint64_t q0, uint32_t n_rows, uint32_t n_out, uint32_t mc, MscEpilogueArgs& e) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	if (!c.reject || !cands->rj_ranges) return MSC_OK;
	int32_t* out = (int32_t*)ctx->reject_cut.p + q0;
	unsigned long long* words = (unsigned long long*)((uint8_t*)ctx->open_words.p + kRejectWordsAt);
	const MscFoldRejectCut a{c.model->d, cands->rj_ranges, cands->L.nbins, cands->dtype, c.order, dq_slots, n_rows, n_out, qset->scalars, qset->scalar_stride, qset->rk_dev, qset->kbf_x,
	                         qset->mb, qset->mb_n, qset->mb_pitch, out, words};
	HIP_TRY(ctx, msc_launch_fold_reject_cut(tail, a));
	e.fold_cut = out; e.fold_cut_words = words;
	ctx->reject_seen += (uint64_t)n_rows * mc; ctx->reject_m = c.m;
	return MSC_OK;
}

// The folded tail: the screen over intervals, the listed pairs' exact counts, their walk and FP64 evaluation. Should ITS list overflow -- every related pair is
// on it, the lower bound of P1 being 0 --, k_emd_list_close raises the block's word of ctx->fold_over and rerun_overflowed, once the call's blocks are through,
// scores the block again with the true product (no host wait here, and nothing queued for the case that did not arise)
int tail_folded(MultiCall& c, Block& b, const MatrixBlock& p, const Chunk& k, uint32_t open_cap, Tail& t) {
	msc_ctx* ctx = c.ctx;
	uint32_t* open_words = (uint32_t*)ctx->open_words.p;
	int r;
	if ((r = ensure_open_list(ctx, open_cap)) || (r = tail_ready(c, b, p, k, t))) return r;
	MscEpilogueArgs ef = bound_args(c, t.ea, open_cap);
	ef.kb_slices = p.slices_f; ef.fold_x_c = c.cands->kbf_x; ef.fold_x_q = c.qset->kbf_x;
	if ((r = cut_rows(c, b.tail, b.dq_slots, b.q0, (uint32_t)b.nq, (uint32_t)b.nq, k.mc, ef))) return r;
	if ((r = list_stage(c, b, p, k, ef, open_cap))) return r;
	HIP_TRY(ctx, msc_launch_emd_list_close(b.tail, open_words, open_cap, (uint64_t*)(open_words + 2), (uint32_t*)ctx->fold_over.p + b.idx));
	return MSC_OK;
}

// the flags' way home: from the chunk's buffer on the copy stream, under the next block's kernels
int flags_home(MultiCall& c, Block& b, const Chunk& k, const Tail& t) {
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	HIP_TRY(ctx, hipEventRecord(pipe.ev_scored[t.pp], b.tail));
	HIP_TRY(ctx, hipStreamWaitEvent(pipe.copy_stream, pipe.ev_scored[t.pp], 0));
	HIP_TRY(ctx, rows_home(b.close + k.off, c.m, t.d_close, (size_t)k.mc, b.nq, pipe.copy_stream));
	HIP_TRY(ctx, hipEventRecord(pipe.ev_copied[t.pp], pipe.copy_stream));
	pipe.close_pp_busy[t.pp] = true;
	pipe.copy_pending = true;
	return MSC_OK;
}

// msc_last_emd_walk / msc_last_fold_screen: what a chunk adds to the call's counters (the overflows are on the device until the call ends)
void count_chunk(msc_ctx* ctx, const MscMatrixStages& st, const MscMatrixChunk& ck) {
	if (!st.counted) return;
	if (st.walk_counted) { ctx->walk_blocks++; if (ck.bounds) ctx->walk_bound_blocks++; else ctx->walk_dense++; }
	if (ck.tail == MSC_TAIL_FOLDED) { ctx->fold_used = st.fold; ctx->fold_blocks++; }
}

// The folded tail of a whole tail group, issued by its last block b: behind ONE wait for that block's product (the stream ran the group's products in order), the
// kernels of tail_folded once, blockIdx.y the block of the group (the first block's arguments and the strides of the group's side and of its query group's arena);
// the lists are closed in block order, the close counts run over the group's rows, and the group's flags -- rows q0 .. of consecutive blocks, contiguous on
// both sides -- go home in one copy on the copy stream. Lists, their words and the fold_over words stay per block: rerun_overflowed sees what it always saw.
int group_tail(MultiCall& c, const Block& b, const MatrixBlock& p, const Chunk& k, uint32_t open_cap) {
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	const MscLayout& L = cands->L;
	const MscTailGroup& T = c.tgroups[p.tgroup];
	const MscQueryGroup& G = c.groups[p.group];
	BlockPipe::GroupSide& g = pipe.gside[c.tgroup_side[p.tgroup]];
	hipStream_t tail = pipe.tail_stream;
	uint8_t* base = (uint8_t*)g.buf.p;
	if (open_cap != T.list_cap || open_cap > T.list_stride) return fail(ctx, MSC_ERR_HIP, "a tail group's lists are not of the capacity it was planned with");
	Block b0 = block_of(c, T.first);
	b0.dq_slots = (const uint32_t*)ctx->qslots_all.p + b0.q0;
	uint32_t* words = (uint32_t*)(base + T.words_off);
	if (g.copy_busy) HIP_TRY(ctx, hipStreamWaitEvent(tail, g.ev_copied, 0));          // (the flags of the group that had this side before are home)
	HIP_TRY(ctx, hipStreamWaitEvent(tail, g.ev_product, 0));
	HIP_TRY(ctx, hipMemsetAsync(words, 0, T.n * T.words_stride * sizeof(uint32_t), tail));
	MscEpilogueArgs ea;
	fill_block_args(c, b0, b0.dq_slots, k, L.S, ea);
	ea.kb_min = (const int32_t*)(base + T.min_off);
	ea.kb_diff = T.diff_stride ? (const int32_t*)(base + T.diff_off) : nullptr;
	ea.kb_slices = p.slices_f; ea.kb_qn = p.rows; ea.kb_first = c.cand_slots ? 0 : k.off;
	ea.kb_c_mb = cands->mb; ea.kb_c_mb_n = cands->mb_n; ea.kb_c_pitch = cands->mb_pitch;
	ea.kb_q_mb = qset->mb; ea.kb_q_mb_n = qset->mb_n; ea.kb_q_pitch = qset->mb_pitch;
	ea.kb_qT = p.qT - (b.idx - T.first) * G.qt_stride;
	ea.emd_stride = p.rows;
	ea.cq_group = 16;
	ea.close_soa = base + T.flags_off;
	ea.screen = p.st.screen;
	ea.rk_c_sum = cands->rk_sum; ea.rk_c_dev = cands->rk_dev; ea.rk_q_sum = qset->rk_sum; ea.rk_q_dev = qset->rk_dev;
	ea.open_list = (uint32_t*)(base + T.list_off); ea.open_words = words; ea.open_cap = open_cap; ea.emd_list = (const uint64_t*)(base + T.emd_off);
	ea.fold_x_c = cands->kbf_x; ea.fold_x_q = qset->kbf_x;
	ea.tg_blocks = (uint32_t)T.n;
	ea.tg_min_stride = T.min_stride; ea.tg_diff_stride = T.diff_stride; ea.tg_qt_stride = G.qt_stride; ea.tg_flags_stride = T.flags_stride;
	ea.tg_list_stride = T.list_stride; ea.tg_q_stride = 128; ea.tg_words_stride = (uint32_t)T.words_stride;
	const MscListGroup lg{(uint32_t)T.n, 128, (uint32_t)T.words_stride, T.list_stride, G.qt_stride, T.min_stride, T.diff_stride};
	const bool u16 = cands->ranks16 && qset->ranks16;
	int r;
	if ((r = cut_rows(c, tail, b0.dq_slots, b0.q0, (uint32_t)std::min<uint64_t>(T.n * 128, c.n_q - b0.q0), (uint32_t)(T.n * 128), k.mc, ea))) return r;
	HIP_TRY(ctx, msc_launch_epilogue_bound(tail, ea));
	const MscFoldExact fx{cands->ranks, cands->rk_pitch, L.nbins, L.E, L.R, k.d_slots, k.off, k.mc, b0.dq_slots, ea.open_list, words, open_cap, ea.kb_qT, p.rows,
	                      qset->mb, qset->mb_n, qset->mb_pitch, (int32_t*)(base + T.min_off), ea.kb_slices, T.diff_stride ? (int32_t*)(base + T.diff_off) : nullptr};
	HIP_TRY(ctx, msc_launch_fold_exact_list(tail, fx, ctx->num_cus, &lg));
	HIP_TRY(ctx, msc_launch_emd_ranks_list(tail, u16, u16 ? (const void*)cands->ranks16 : (const void*)cands->ranks, u16 ? (const void*)qset->ranks16 : (const void*)qset->ranks,
	                                       cands->rk_pitch, k.d_slots, k.off, k.mc, b0.dq_slots, ea.open_list, words, open_cap, (uint64_t*)(base + T.emd_off), ctx->num_cus, &lg));
	HIP_TRY(ctx, msc_launch_epilogue_list(tail, ea, ctx->num_cus));
	HIP_TRY(ctx, msc_launch_emd_list_close(tail, words, open_cap, (uint64_t*)((uint32_t*)ctx->open_words.p + 2), (uint32_t*)ctx->fold_over.p + T.first, (uint32_t)T.n, (uint32_t)T.words_stride));
	if (ctx->close_counts_n) HIP_TRY(ctx, msc_launch_close_counts(tail, ea.close_soa, (uint32_t)(T.n * 128), k.mc, (uint64_t*)ctx->close_counts.p + b0.q0));
	HIP_TRY(ctx, hipEventRecord(g.ev_tail, tail));
	g.tail_busy = true;
	pipe.tail_used = true;
	HIP_TRY(ctx, hipStreamWaitEvent(pipe.copy_stream, g.ev_tail, 0));
	HIP_TRY(ctx, hipMemcpyAsync(b0.close, ea.close_soa, T.n * T.flags_stride, hipMemcpyDeviceToHost, pipe.copy_stream));
	HIP_TRY(ctx, hipEventRecord(g.ev_copied, pipe.copy_stream));
	g.copy_busy = true;
	pipe.copy_pending = true;
	ctx->tail_group_runs++; ctx->tail_group_blocks += T.n;
	return MSC_OK;
}

// candidates [off, off + b.chunk) of the block: the product, one of the three tails, the results' way home
int matrix_chunk(MultiCall& c, Block& b, const MatrixBlock& p, uint64_t off) {
	msc_ctx* ctx = c.ctx;
	BlockPipe& pipe = ctx->pipe;
	BlockPipe::Side& s = *p.s;
	const bool queued = p.rt->queued;
	int r;
	const Chunk k = chunk_at(c, b, off);
	hipEvent_t ev_t0 = ctx->ev_tiles0, ev_t1 = ctx->ev_tiles1;
	if (queued && ctx->timing && ((r = pool_event(ctx, &ev_t0)) || (r = pool_event(ctx, &ev_t1)))) return r;      // (read when the call's last block is through)
	if ((r = product_stage(c, b, p, k, ev_t0, ev_t1))) return r;
	const MscMatrixChunk ck = msc_matrix_chunk(p.st, b.nq, k.mc);
	count_chunk(ctx, p.st, ck);
	if (p.tgroup >= 0) {          // the tail is its group's: issued behind the product of the group's last block
		const MscTailGroup& T = c.tgroups[p.tgroup];
		if (b.idx + 1 == T.first + T.n && (r = group_tail(c, b, p, k, ck.open_cap))) return r;
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all1, ctx->stream));
		ctx->tiles_launches++;
		return MSC_OK;
	}
	Tail t;
	switch (ck.tail) {
		case MSC_TAIL_SCORED: r = tail_scored(c, b, p, k, t); break;
		case MSC_TAIL_BOUNDS: r = tail_bounds(c, b, p, k, ck.open_cap, t); break;
		case MSC_TAIL_FOLDED: r = tail_folded(c, b, p, k, ck.open_cap, t); break;
	}
	if (r) return r;
	if (b.close && ctx->close_counts_n) HIP_TRY(ctx, msc_launch_close_counts(b.tail, t.d_close, (uint32_t)b.nq, k.mc, (uint64_t*)ctx->close_counts.p + b.q0));
	if (p.st.piped) {
		HIP_TRY(ctx, hipEventRecord(s.ev_tail, b.tail));
		s.tail_busy = true;
		pipe.tail_used = true;
	}
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all1, ctx->stream));
	if ((r = results_home(c, b, k))) return r;
	if (b.close && (r = flags_home(c, b, k, t))) return r;
	if (queued) ctx->tiles_launches++;
	else if ((r = chunk_done(ctx, ev_t0, ev_t1))) return r;
	return MSC_OK;
}

// second_run: the block ran folded and its list overflowed -- it runs again with the true product (rerun_overflowed)
int run_matrix(MultiCall& c, Block& b, const BlockRoute& rt, bool second_run = false) {
	msc_ctx* ctx = c.ctx;
	const uint64_t nbins = c.cands->L.nbins;
	int r;
	if ((r = begin_block(ctx)) || (r = block_uploads(c, b, rt.queued))) return r;
	const uint32_t rows = settle_matrix_block(c, b);
	if ((r = ensure_block_scratch(c, b, true))) return r;
	MatrixBlock p = plan_matrix(c, b, rt, rows, second_run);
	p.group = second_run || c.group_of.empty() ? -1 : c.group_of[b.idx];
	if (p.group >= 0 && (!p.st.piped || rows != 128 || p.st.fold != c.groups[p.group].fold)) return fail(ctx, MSC_ERR_HIP, "a grouped block's stages are not those its group was planned with");
	p.tgroup = p.group < 0 || c.tgroup_of.empty() ? -1 : c.tgroup_of[b.idx];
	if (p.tgroup >= 0 && (msc_matrix_chunk(p.st, b.nq, c.m).tail != MSC_TAIL_FOLDED || b.chunk != c.m)) return fail(ctx, MSC_ERR_HIP, "a block's tail is not the one its tail group was planned with");
	if (p.tgroup < 0 && (r = wait_side_free(ctx, p))) return r;
	// (a folded block passes the true bin count and the larger of the two slice counts)
	if (p.tgroup >= 0) {
		if ((r = tail_group_slot(c, b, p)) || (r = group_side(c, b, p))) return r;
	} else if (p.group >= 0) {
		if ((r = ensure_products(ctx, *p.s, rows, std::max(p.slices, p.slices_f), b.chunk, rt.n_hot)) || (r = group_side(c, b, p))) return r;
	} else {
		if ((r = ensure_side(ctx, *p.s, nbins, rows, std::max(p.slices, p.slices_f), b.chunk, rt.n_hot, &p.hot)) || (r = queries_side(c, b, p))) return r;
		p.qT = (const uint8_t*)p.s->qT.p; p.anib = (const uint8_t*)p.s->anib.p; p.hot_entries = p.s->hot.p;
	}
	if (p.tgroup < 0) { p.out_min = (int32_t*)p.s->min.p; p.out_diff = (int32_t*)p.s->diff.p; }
	if (rt.emd_ranks && (r = ensure(ctx, ctx->emd_out, b.chunk * rows * sizeof(uint64_t)))) return r;
	name_matrix_kernel(ctx, rows, rt.emd_ranks, c.cells, c.cands->sparse, p.st.fold);
	ctx->last_query_tile = (int)b.nq;
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all0, ctx->stream));
	if (c.reject && p.st.fold && (r = ensure_reject_ranges(ctx, c.cands))) return r;          // (ahead of the product: the tail that reads them waits for it)
	for (uint64_t off = 0; off < c.m; off += b.chunk)
		if ((r = matrix_chunk(c, b, p, off))) return r;
	return rt.queued ? MSC_OK : read_error_word(ctx);
}

// What the older routes need of two dense sets when a divergence or group statistic is wanted: the sparse mirrors, both or neither, and with them
// whether a block of two or more can run on one of the Q x M kernels (c.simple).
int settle_mirrors(MultiCall& c) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	const MscLayout& L = cands->L;
	int r;
	c.mirrors_settled = true;
	const bool whole_tiles = L.nbins == L.padded_bins && !needs_wide(cands, qset);
	if ((c.want_div || c.want_grp) && !cands->sparse && c.n_q > 1 && whole_tiles) {
		if ((r = ensure_sparse_mirror(ctx, cands, &c.c_sp)) || (r = ensure_sparse_mirror(ctx, qset, &c.q_sp))) return r;
		if (!c.c_sp || !c.q_sp) c.c_sp = c.q_sp = nullptr;
	}
	c.grp_dense = c.want_grp && !c.c_sp;
	c.simple = !cands->sparse && (!c.grp_dense || c.mc_ <= 0xffffffffull) && (!c.want_div || c.c_sp) && whole_tiles;
	return MSC_OK;
}

// block i of the call's plan
Block block_of(const MultiCall& c, size_t i) {
	const MscMultiBlock& pb = c.blocks[i];
	const uint64_t m = c.m;
	Block b{pb.q0, pb.nq, c.q_slots + pb.q0, c.sum_out ? c.sum_out + pb.q0 * m : nullptr, c.csum_out ? c.csum_out + pb.q0 * m : nullptr,
	        c.raw_out ? c.raw_out + pb.q0 * m * c.nf : nullptr, c.close_out ? c.close_out + pb.q0 * m : nullptr};
	b.idx = (uint32_t)i;
	return b;
}

// The folded blocks whose list overflowed (msc_fold.h): once more, as the unfolded blocks they would have been -- the bounds of emd, the list, the dense
// walk behind it. The call's streams are idle; the block's close counts start again from zero, its flags go home over the first run's
int rerun_overflowed(MultiCall& c, const std::vector<BlockRoute>& route_of) {
	msc_ctx* ctx = c.ctx;
	int r;
	std::vector<uint32_t> over(c.blocks.size());
	HIP_TRY(ctx, hipMemcpy(over.data(), ctx->fold_over.p, over.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
	for (size_t i = 0; i < over.size(); i++) {
		if (!over[i]) continue;
		Block b = block_of(c, i);
		if (ctx->close_counts_n) HIP_TRY(ctx, hipMemsetAsync((uint64_t*)ctx->close_counts.p + b.q0, 0, b.nq * sizeof(uint64_t), ctx->stream));
		if ((r = run_matrix(c, b, route_of[i], true))) { (void)flush_deferred(c); return r; }
		c.ms += ctx->tiles_ms_accum; c.launches += ctx->tiles_launches;
	}
	return flush_deferred(c);
}

// The call's counters (msc_last_emd_walk, msc_last_fold_screen) start from zero ...
void clear_call_counters(msc_ctx* ctx) {
	ctx->walk_listed = ctx->walk_dense = ctx->walk_blocks = ctx->walk_bound_blocks = ctx->fold_used = ctx->fold_blocks = ctx->fold_fell_back = 0;
	ctx->tail_group_runs = ctx->tail_group_blocks = 0;
	ctx->reject_seen = ctx->reject_m = ctx->reject_pairs = ctx->reject_rows_none = 0;
}

// ... and take the totals of the bound pass when the call is through (every stream of the call is idle: the error word has been read)
int read_call_totals(msc_ctx* ctx, const msc_model* model) {
	if (!ctx->walk_bound_blocks) return MSC_OK;
	uint64_t totals[5] = {0, 0, 0, 0, 0};          // (a folded block is a bound block: the cut's two words come home in the same copy)
	const hipError_t e = hipMemcpy(totals, (const uint8_t*)ctx->open_words.p + 2 * sizeof(uint32_t), sizeof totals, hipMemcpyDeviceToHost);
	if (e != hipSuccess) return fail(ctx, MSC_ERR_HIP, "copy of the pair list's totals failed: %s", hipGetErrorString(e));
	ctx->walk_listed = totals[0];
	ctx->walk_dense += totals[1];
	// a model whose distance really decides: it does not pay the bound pass for ever
	if (totals[1] * 2 > ctx->walk_bound_blocks) model->emd_decides = true;
	// ... nor, a model whose related pairs are too many for the list, the folded stage
	ctx->fold_fell_back = totals[2];
	if (totals[2] * 2 > ctx->fold_blocks) model->fold_overflows = true;
	if (ctx->reject_seen) {          // msc_last_fold_reject: the pairs of the rows that had a cut, less those the screen evaluated all the same
		ctx->reject_rows_none = totals[4];
		ctx->reject_pairs = ctx->reject_seen - totals[4] * ctx->reject_m - totals[3];
	}
	return MSC_OK;
}

// The device words the call's blocks add into, cleared on the context's stream: close candidates per query, kept for msc_last_close_counts (a caller that
// only needs the counts of a block of the pairwise matrix does not have to add up n_q x m flags on the host) ...
int clear_call_words(MultiCall& c) {
	msc_ctx* ctx = c.ctx;
	const uint64_t n_q = c.n_q;
	int r;
	ctx->close_counts_n = 0;
	if (c.close_out && c.model) {          // the list of open pairs of the bound pass (run_matrix): {count, overflow}, then the call's two totals
		// (+ the third total, folded blocks that fell back; and per block of the plan a word that a folded block raises when its list overflows)
		if ((r = ensure(ctx, ctx->open_words, kOpenWordsBytes))) return r;
		HIP_TRY(ctx, hipMemsetAsync(ctx->open_words.p, 0, kOpenWordsBytes, ctx->stream));
		const size_t over_bytes = ((n_q + 63) / 64 + 1) * sizeof(uint32_t);          // (a plan's blocks are of 64 queries or more, but for the last)
		if ((r = ensure(ctx, ctx->fold_over, over_bytes))) return r;
		HIP_TRY(ctx, hipMemsetAsync(ctx->fold_over.p, 0, over_bytes, ctx->stream));
	}
	if (c.reject) {          // the cut of every query row of the call (whole blocks of 128); its two counters are words of open_words, cleared above
		if ((r = ensure(ctx, ctx->reject_cut, (n_q + 127) / 128 * 128 * sizeof(int32_t)))) return r;
	}
	if (c.close_out) {
		if ((r = ensure(ctx, ctx->close_counts, n_q * sizeof(uint64_t)))) return r;
		HIP_TRY(ctx, hipMemsetAsync(ctx->close_counts.p, 0, n_q * sizeof(uint64_t), ctx->stream));
		ctx->close_counts_n = n_q;
	}
	return MSC_OK;
}

// validate, decide kb_fit once, plan the blocks, run each on its route, wait for what was queued
int score_multi(MultiCall& c) {
	msc_ctx* ctx = c.ctx;
	const msc_hist_set *cands = c.cands, *qset = c.qset;
	const uint64_t n_q = c.n_q, m = c.m;
	if (!ctx || !cands || !qset || !c.q_slots || (c.model && c.model->ctx != ctx)) return MSC_ERR_INVALID_ARG;
	if (c.raw_out && (c.feat_mask == 0 || (c.feat_mask & ~kSupportedFeats))) return fail(ctx, MSC_ERR_UNSUPPORTED, "feat_mask holds statistics outside the GPU path");
	if (!c.raw_out) c.feat_mask = 0;
	if (n_q == 0 || m == 0) return MSC_OK;
	for (uint64_t i = 0; i < n_q; i++) if (c.q_slots[i] >= qset->capacity) return fail(ctx, MSC_ERR_INVALID_ARG, "query slot out of range");
	int r = validate_pair(ctx, cands, qset, c.q_slots[0], c.cand_slots, m);
	if (r) return r;
	const MscLayout& L = cands->L;
	c.nf = __builtin_popcountll(c.feat_mask);
	c.want = c.feat_mask;
	if (c.model) for (int i = 0; i < c.model->h.n_singles; i++) c.want |= c.model->h.single_flag[i];
	c.need_emd = (c.want & MSC_FEAT_EMD) != 0;           // Feature::compute evaluates only the model's singles too
	c.want_div = (c.want & MSC_FEAT_DIV) != 0; c.want_grp = (c.want & MSC_FEAT_GROUPS) != 0;
	// The pass on the matrix cores (msc_pair_gemm.hip) serves blocks of up to 128 queries per pass over the candidates' bits; the older routes 64
	// A divergence statistic without a group statistic, under msc_set_multi_div_cells (div_cells): the epilogue forms the two sums from cells (bits_pair_div,
	// pair_features.hip) and no pass runs between the product and it -- dense sets, and two sparse sets under msc_set_sparse_matrix_pass. Any other divergence
	// or group statistic: dense sets queue their passes behind the product, two sparse sets keep the call on the merge kernels, blocks of 64 and all
	const bool div_cells = ctx->multi_div_cells && c.want_div && !c.want_grp;
	c.kb_fit = n_q >= 2 && kb_route_fits(cands, qset, c.need_emd) && !(cands->sparse && (c.want_grp || (c.want_div && !div_cells)));
	if (c.kb_fit) {
		const bool flags_only = c.model && c.close_out && !c.sum_out && !c.csum_out && !c.raw_out && c.need_emd && !c.want_div && !c.want_grp;
		if ((r = ensure_kb(ctx, cands, flags_only)) || (r = ensure_kb(ctx, qset, flags_only))) return r;
		c.kb_fit = cands->kb && qset->kb && !cands->kb_has_zero && !qset->kb_has_zero;
		c.reject = ctx->fold_reject && flags_only && c.kb_fit && c.model->h.screen_ok && reject_ranges_cover(cands, c.cand_slots, m);
	}
	c.cells = div_cells && c.kb_fit;
	if ((r = clear_call_words(c))) return r;
	c.mc_ = std::max(cands->max_count, qset->max_count); c.ms_ = std::max(cands->max_sum, qset->max_sum);
	// (sums from cells read no sparse mirror: a call whose blocks all stay with the matrix cores builds none; the first block that falls back settles them)
	if (c.cells) c.simple = !cands->sparse;
	else if ((r = settle_mirrors(c))) return r;
	// wave totals of the per-lane 32-bit partial sums fit 32 bits when 64*R*max^2 and 64*R*max|prefix difference| do
	c.compact = 64ull * L.R * c.mc_ * c.mc_ < (1ull << 32) && 64ull * L.R * c.ms_ < (1ull << 32);
	// every prefix of excess counts (count - 1) is at most the histogram's k-mer total = sum - 4^k: 16-bit prefix form when that fits
	c.excess16 = c.ms_ >= L.nbins && c.ms_ - L.nbins < 65536;
	int err = MSC_OK;
	msc_multi_plan(n_q, c.kb_fit, [&](uint64_t q0, uint64_t nq) {
		const BlockRoute rt = err ? BlockRoute() : pick_route(c, c.q_slots + q0, nq, true, &err);
		if (rt.kind == R_MATRIX) c.taken.push_back(rt);
		return rt.kind != R_MATRIX;
	}, c.blocks);
	if (err) return err;
	plan_query_groups(c);
	plan_tail_groups(c);
	size_t next_taken = 0;
	std::vector<BlockRoute> route_of(c.blocks.size());
	for (size_t i = 0; i < c.blocks.size(); i++) {
		const MscMultiBlock& pb = c.blocks[i];
		Block b = block_of(c, i);
		// (blocks of the matrix-core pass are queued without a host wait between them: any other route first waits for them and reads their error word)
		r = pb.matrix ? MSC_OK : flush_deferred(c);
		BlockRoute rt;
		if (pb.matrix) rt = c.taken[next_taken++];
		else {
			if (!r && !c.mirrors_settled) r = settle_mirrors(c);          // (sums from cells, and this block falls back)
			if (!r) rt = pick_route(c, b.q_slots, b.nq, false, &r);
		}
		if (!r && rt.queued && !c.queue_up) {          // the first queued block: the whole call's query slots go up once
			if (!(r = ensure(ctx, ctx->qslots_all, n_q * sizeof(uint32_t)))) {
				HIP_TRY(ctx, hipMemcpyAsync(ctx->qslots_all.p, c.q_slots, n_q * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
				HIP_TRY(ctx, hipEventRecord(ctx->pipe.ev_call, ctx->stream));
				ctx->pipe.ev_used = 0; c.queue_up = true;
			}
		}
		route_of[b.idx] = rt;
		if (!r) switch (rt.kind) {
			case R_MATRIX: r = run_matrix(c, b, rt); break;
			case R_DIGEST: case R_RING: case R_TILES: r = run_streamed(c, b, rt); break;
			case R_SPARSE_QUEUED: r = run_sparse_queued(c, b); break;
			case R_PER_QUERY: r = run_per_query(c, b); break;
		}
		if (r) { (void)flush_deferred(c); return r; }          // (nothing of this call may still be running when it returns)
		c.ms += ctx->tiles_ms_accum; c.launches += ctx->tiles_launches;
	}
	if ((r = flush_deferred(c))) return r;
	if (ctx->fold_blocks && (r = rerun_overflowed(c, route_of))) return r;
	ctx->tiles_ms_accum = c.ms; ctx->tiles_launches = c.launches;
	return MSC_OK;
}

}  // namespace

extern "C" int msc_score_multi(msc_ctx* ctx, const msc_model* model, const msc_hist_set* cands, const uint32_t* cand_slots, uint64_t m,
                               const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q, int order, double* sum_out, double* csum_out,
                               uint8_t* close_out, uint64_t feat_mask, double* raw_out) {
	MultiCall c{ctx, model, cands, cand_slots, m, qset, q_slots, n_q, order, sum_out, csum_out, close_out, feat_mask, raw_out};
	if (ctx) clear_call_counters(ctx);
	int r = score_multi(c);
	if (ctx && r == MSC_OK) r = read_call_totals(ctx, model);
	if (ctx && ctx->pipe.copy_pending) {          // the flag copies of the last blocks (issued beside the kernels that followed them)
		const hipError_t e = hipStreamSynchronize(ctx->pipe.copy_stream);
		ctx->pipe.copy_pending = ctx->pipe.close_pp_busy[0] = ctx->pipe.close_pp_busy[1] = ctx->pipe.gside[0].copy_busy = ctx->pipe.gside[1].copy_busy = false;
		if (e != hipSuccess && r == MSC_OK) return fail(ctx, MSC_ERR_HIP, "copy of the close flags failed: %s", hipGetErrorString(e));
	}
	return r;
}
