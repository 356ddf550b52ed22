// msc_objects.h -- the objects behind the opaque handles of include/meshclust2_hip.h and the host helpers the C-ABI translation
// units share (msc_api*.hip define them; msc_window.hip and msc_shard.hip use them). Private to the library.
#pragma once
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "msc_internal.h"

struct DevBuf {
	void* p = nullptr;
	size_t cap = 0;
};

// The matrix-core block pipe (msc_pair_gemm.hip; run_matrix and its stage functions, msc_api_multi.hip). msc_score_multi queues the blocks of its matrix-core pass in stages on three
// streams: the queries' side of block i + 1 (prep_stream) under the product of block i (the context's stream), beside the rank walk of block i and the
// epilogue of block i - 1 (tail_stream). What two stages touch exists twice and blocks take turns; msc_search_pairs, on one stream, uses side[0] alone.
// Consecutive piped blocks of 128 rows form GROUPS (msc_set_query_groups, msc_query_groups in msc_multi_plan.h): the queries' side of a whole group is one
// set of launches into one of two arenas, issued once on prep_stream while the blocks of the group before run -- the products of the group wait for it
// once (ev_ready), and the arena is rewritten behind the product and the tail of the last block that read it. A grouped block's qT, anib and hot list are
// views into the arena; its side keeps min and diff, and what remains per block is the product, the tail and the flags' way home:
//
//   prep_stream   | side of group g + 1 (arena 1)          | side of group g + 2 (arena 0) ...
//   the stream    | product g.0 | product g.1 | ... | product g.n-1 | product g+1.0 | ...
//   tail_stream   |             | tail g.0    | tail g.1 ...
struct BlockPipe {
	struct Side {
		// bit image transposed, P1 per slice, P2, the queries' tiles as nibbles (what the product copies into LDS), hot list + its three step arrays
		DevBuf qT, min, diff, anib, hot, hot_idx;
		// the product of a block on this side is about to start / is through, the epilogue that read this side is through, the queries' side is ready
		hipEvent_t ev_head = nullptr, ev_product = nullptr, ev_tail = nullptr, ev_prep = nullptr;
		bool product_busy = false, tail_busy = false;          // a product that reads this side / an epilogue that read it has been queued
	} side[2];
	// the queries' side of a group of blocks: its images and lists (msc_query_groups lays them out); ready: the group's side is through; last: the side of
	// the pipe the last block that reads the arena took (its ev_product and ev_tail), busy: such a block has been queued
	struct Arena {
		DevBuf buf;
		hipEvent_t ev_ready = nullptr;
		Side* last = nullptr;
		bool busy = false;
	} arena[2];
	uint32_t arena_next = 0;               // the arena the next group takes (its low bit)
	// The folded tail of a TAIL GROUP of blocks in one set of launches (msc_set_tail_groups; msc_tail_groups in msc_multi_plan.h lays a side out): P1, P2, flags,
	// lists and list words of the group's blocks in one buffer, two such sides taking turns. A block of the group issues its product into its slot; the
	// group's last block issues the tail on tail_stream and the flags' copy home on copy_stream. The events are a Side's: ev_product the last product
	// issued into the side, ev_tail the tail that read it; ev_copied the flags' copy
	struct GroupSide : Side {
		DevBuf buf;
		hipEvent_t ev_copied = nullptr;
		bool copy_busy = false;
	} gside[2];
	uint32_t gside_next = 0;               // the side the next tail group takes (its low bit)
	hipStream_t tail_stream = nullptr, prep_stream = nullptr, copy_stream = nullptr;
	hipEvent_t ev_call = nullptr;          // the call's query slots are on the device
	// the close flags of a block go back to the host on copy_stream, under the next block's kernels: two device buffers take turns, and
	// msc_score_multi waits for the copies before it returns
	DevBuf close_pp[2];
	hipEvent_t ev_scored[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
	bool close_pp_busy[2] = {false, false}, copy_pending = false, tail_used = false;
	int close_pp_next = 0;
	uint32_t next = 0;                     // the side the next piped block takes (its low bit)
	std::vector<hipEvent_t> ev_pool;       // timing events of the queued blocks, kept for the life of the context
	size_t ev_used = 0;
};

struct msc_ctx {
	int device = -1;
	int num_cus = 256;
	hipStream_t stream = nullptr;
	hipEvent_t ev_tiles0 = nullptr, ev_tiles1 = nullptr, ev_all0 = nullptr, ev_all1 = nullptr;
	bool have_timing = false;
	bool timing = true;                      // record the HIP events behind msc_last_kernel_ms (msc_set_kernel_timing)
	uint32_t last_partial_stride = 0;        // partial records per candidate written by the last run_score
	float tiles_ms_accum = 0.f;
	int tiles_launches = 0;
	const char* last_kernel = "";            // streaming kernel of the last scoring call
	char last_kernel_buf[160] = "";          // (where the Q x M pass composes the name of the form it ran)
	int last_query_tile = 1;                 // queries one HBM read of a candidate tile served in it
	std::string err;
	char dev_name[128] = {0};
	// growable device scratch
	DevBuf partials, pair_out, flags, reduce_out, slots, raw, singles, combos, packed, seg_seq, seg_start, kmer_off, nat, model_tmp,
	    floor_sum, mean, div_tables, div_partials, qslots, soa_sum, soa_csum, soa_close, err_word, seq_seg, seq_ids, seq_meta;
	DevBuf rk_items;                       // ... its list of (candidate, round) items
	DevBuf rk_acc;                         // ... of its long-list form: a record and a spot-term slot per item (k_pair_ranks_items)
	DevBuf rk_counters;                    // ... 2 x 16 words: the query's counts of counts and the number of items, two sets used in turn
	uint32_t rk_turn = 0;
	DevBuf rk_tables;                      // ... the query's tables as the pass's workgroups copy them into LDS, two sets used in turn
	uint32_t rk_table_words = 0;
	DevBuf rk_big;                         // ... the query's counts of 8 and more, for the divergence statistics of the long-list pass (MscRankDiv)
	DevBuf rk_q;                           // the rank list of a pass's query when it is too long for LDS (msc_ranks_pass.hip)
	uint32_t* rk_guard = nullptr;          // page-locked word the rank pass raises when a query's list is longer than its set's bound (msc_ranks_pass.hip)
	DevBuf pin_mean;                       // page-locked: the small pieces a sparse msc_mean_nearest call hands to and fro (msc_api_score.hip)
	DevBuf pin_parts;                      // page-locked: the parts of the fused epilogue + reduce kernel when the host folds them
	DevBuf pin_up, pin_down;               // page-locked HOST staging of the per-call slot list / reduce record + flags
	msc_hist_set* scratch_set = nullptr;   // one slot: the rounded mean of msc_mean_nearest
	msc_hist_set* sparse_scratch = nullptr; // dense slots the sparse builder compacts from
	DevBuf sp_counts, sp_cumbase, sp_acc, sp_chunk_off, sp_chunk_cum, sp_partials, grp_pairs, grp_self, sp_acc_batch, tile_scratch, reduce_parts, sp_touched;
	msc_hist_set* sparse_mean_set = nullptr;   // one sparse slot: the rounded mean of msc_mean_nearest on sparse members
	msc_hist_set* sparse_mean_batch = nullptr; // the rounded means of one chunk of centres (msc_update_centres on sparse sets)
	msc_hist_set* batch_scratch = nullptr;     // rounded means of one chunk of centres (msc_update_centres)
	DevBuf segs, pair_seg, dist;
	uint64_t sp_acc_bins = 0;
	// msc_shard.hip: the payload of msc_colsum_partial, the gathered column-sum lists of the other ranks, header staging
	DevBuf shard_payload, shard_hdrs;
	BlockPipe pipe;                        // msc_pair_gemm.hip: the queries' side of a block and the streams its stages run on
	bool block_pipe = true;                // msc_set_block_pipe: the blocks of msc_score_multi on three streams
	uint32_t query_groups = 32;            // msc_set_query_groups / MSC_NO_QUERY_GROUPS: most blocks whose queries' side one set of launches builds (0, 1: block by block)
	uint32_t tail_groups = 8;              // msc_set_tail_groups / MSC_NO_TAIL_GROUPS: most folded blocks whose tail one set of launches runs (0, 1: block by block)
	uint64_t tail_group_runs = 0, tail_group_blocks = 0;          // msc_last_tail_groups: the last call's
	bool tail_ramp = true;                 // ... the call's final groups halve down to one block (MSC_TAIL_NO_RAMP: full groups to the end, for A/B runs)
	bool pairs_div_cells = false;          // msc_set_pairs_div_cells: msc_search_pairs keeps divergence-statistic models on the matrix-core route
	bool multi_div_cells = false;          // msc_set_multi_div_cells: msc_score_multi keeps blocks that want a divergence statistic on the matrix-core route, no merge pass
	bool sparse_matrix_pass = false;       // msc_set_sparse_matrix_pass: two sparse sets may take the matrix-core Q x M route (mirrors built from their lists)
	bool mirror_pass = true;               // msc_set_mirror_pass: a dense set's 1 x M passes merge the lists of its sparse mirror
	bool packed_on_device = false;         // msc_hist_build_packed_dev: the 2-bit stream of the build in progress is device memory
	DevBuf close_counts;                   // msc_score_multi: close candidates per query of the call in progress / the last call (msc_last_close_counts)
	// msc_search_pairs (msc_api_pairs.hip): the list of the last call (candidate index, similarity), kept until the next call, and its scratch
	DevBuf pl_idx, pl_sim;
	uint64_t pl_n = 0;                     // pairs in the list
	DevBuf pl_stage_idx, pl_stage_sim;     // a block's pairs chunk by chunk, when its candidates take several chunks
	DevBuf pl_flags, pl_counts, pl_offsets, pl_seg, pl_dst, pl_qslots, pl_win, pl_qcount, pl_words;
	DevBuf pl_pin;                         // page-locked: the running totals read back before a list grows
	// msc_search_pairs_strands: the forward pass's list moved aside, the merged list before it takes the list's place, a strand byte per pair of the
	// list (pl_strands: the last call left one), the three offset arrays, R's r_only words and the merged counts
	DevBuf ps_idx, ps_sim, ps_m_idx, ps_m_sim, pl_strand, ps_off, ps_only, ps_counts;
	bool pl_strands = false;
	msc_hist_set* strand_set = nullptr;    // ... and the queries' reverse complements: n_q slots of the query set's shape, reused and grown between calls
	uint64_t close_counts_n = 0;           // queries the counts on file cover (0: the last call kept none)
	DevBuf qslots_all;                     // msc_score_multi: the query slots of a whole call whose blocks are queued
	DevBuf emd_out, rk_bad;                // msc_emd_ranks.hip: the distances of a chunk, the build's error word
	// msc_emd_list.hip: the pairs of a block whose close flag the bounds of the distance leave open, their exact distances, and the words
	// {count, overflow} (uint32) + {pairs walked, blocks that overflowed} (uint64, the call's totals) of that list
	DevBuf open_list, emd_list, open_words;
	DevBuf fold_over;                      // msc_fold.h: per block of a msc_score_multi call a word its folded stage raises when its list overflows
	bool emd_bounds = true;                // msc_set_emd_bounds / MSC_NO_EMD_BOUNDS: close flags from bounds of the distance, rank walk for the open pairs only
	uint64_t walk_listed = 0, walk_dense = 0, walk_blocks = 0;          // msc_last_emd_walk: the last msc_score_multi call
	uint64_t walk_bound_blocks = 0;        // ... its blocks that took the bound pass (their overflows are on the device until the call ends)
	// msc_set_fold_screen / MSC_NO_FOLD (msc_fold.h): 0, or the fold of the product of such blocks (8, 16, 32); msc_last_fold_screen: the last call's
	// fold, its blocks whose product was folded, and those of them whose list overflowed (scored again with the true product)
	uint32_t fold_screen = 16;
	uint64_t fold_used = 0, fold_blocks = 0, fold_fell_back = 0;
	// msc_set_fold_reject / MSC_NO_FOLD_REJECT (msc_fold_reject.h): the integer cut of a folded block's rows. reject_cut: T per query row of the call in progress;
	// its two counters {pairs evaluated in rows with a cut, rows without a cut} are the last words of open_words, on the device until the call ends; reject_seen: the pairs of the folded
	// blocks that ran with cuts; msc_last_fold_reject: the last call's pairs the cut rejected and rows without a cut
	bool fold_reject = true;
	DevBuf reject_cut;
	uint64_t reject_seen = 0, reject_m = 0, reject_pairs = 0, reject_rows_none = 0;          // (reject_m: the candidates of the call)
	msc_hist_set* shard_gather = nullptr;
	// msc_align_pairs (msc_align.hip): the sequences of a call, its sorted pair records, the three result arrays, and the carry columns of the pairs
	// too long for LDS
	DevBuf align_text, align_pairs, align_out, align_carry, align_band_pairs;          // (align_band_pairs: the records of msc_align_band.hip's rounds)
	DevBuf align_long_pairs, align_long_tiles, align_long_borders;          // msc_align_long.hip: a round's pair records, its tile table, the pairs' borders
	// msc_align_pairs_trace (msc_align_trace.hip): a group's back pointers, where each of its pairs' start, the call's range ends and run counts,
	// and the op list of the last call (align_trace_n words), kept until the next call
	DevBuf align_trace_dirs, align_trace_at, align_trace_idx, align_trace_ops;
	uint64_t align_trace_n = 0;
	// MSC_PROFILE_CALLS: host wall clock of the 1 x M scoring calls, split into preparing + queueing the slot list, issuing the
	// launches, and waiting for the stream (printed by msc_destroy)
	double prof_prep = 0, prof_issue = 0, prof_wait = 0;
	DevBuf prof_nnz;                       // {stored bins, candidates} the list passes scored inside their windows (device counters)
	double prof_tiles_ms = 0;              // streaming-kernel time of those passes (HIP events; needs kernel timing on)
	uint64_t prof_q_nnz = 0;               // sum over the passes of the query's stored bins
	uint64_t prof_calls = 0, prof_cands = 0;
};

// the slots of a set one of its mirrors has not seen written yet: their hull [lo, hi)
struct StaleRange {
	uint64_t lo = 0, hi = 0;
	bool any() const { return lo < hi; }
	void add(uint64_t first, uint64_t n) {
		if (n) *this = any() ? StaleRange{std::min(lo, first), std::max(hi, first + n)} : StaleRange{first, first + n};
	}
	void all(uint64_t capacity) { lo = 0; hi = capacity; }
	void clear() { lo = hi = 0; }
};

// fn(first, n) for every run of consecutive slots i of [lo, hi) with holds(i); the first status other than 0 ends the walk and is returned
template <class Holds, class Fn>
inline int for_each_run(uint64_t lo, uint64_t hi, Holds holds, Fn fn) {
	for (uint64_t i = lo, j; i < hi; i = j) {
		for (j = i; j < hi && holds(j);) j++;
		if (j == i) j++;
		else if (const int r = fn(i, j - i)) return r;
	}
	return 0;
}

struct msc_hist_set {
	msc_ctx* ctx = nullptr;
	int k = 0, dtype = 0;
	uint64_t capacity = 0;
	MscLayout L;
	uint64_t scalar_stride = 0;
	uint8_t* bins = nullptr;
	uint8_t* scalars = nullptr;
	// host-side bounds over every slot ever written (monotone; used to pick the kernels' integer range)
	uint64_t max_count = 0, max_sum = 0;
	const char* last_builder = "";        // what the last msc_hist_build* call on this set ran (msc_hist_set_build_info)
	// digest mirror (pair_digest.hip), allocated on the first Q x M pass that can use it; dg_stale: the slots written since
	mutable uint8_t* digest = nullptr;    // a cache: maintained through const handles
	mutable StaleRange dg_stale;
	mutable bool digest_unavailable = false;      // allocation failed once: do not retry every pass
	// presence-bit mirror (msc_pair_gemm.hip, msc_kbits.h): one BIT per bin = [count >= 2], slots blocked by 32 -- the B operand of the
	// int8 product of the Q x M pass -- and beside it the lists of large bins (count - 1 >= 2) that make the pass exact for any counts:
	// mb[slot][mb_pitch] = (bin, count - 1), sorted by bin; mb_n = entries per slot (also on the host: the size of a query block's hot list is
	// known without a read-back). kb_stale: the slots written since (mark_stale, msc_mirrors.hip). A sparse set carries the same mirror, built from its lists
	// (msc_set_sparse_matrix_pass; lists_written keeps the stale range)
	mutable uint8_t* kb = nullptr;
	mutable StaleRange kb_stale;
	mutable bool kb_unavailable = false;
	mutable bool kb_has_zero = false;         // a slot with a zero count went into the mirror (never the case for built histograms and their means)
	// ... and the mirror folded F-to-1 (msc_fold.h; k_kb_fold): a bit per folded bin in kb's own layout at 4^k / kbf_fold bins, and per slot its own
	// collisions kbf_x. Built from kb in ensure_kb_folded (msc_mirrors.hip) wherever kb is (re)built: kbf_stale = the slots kb has been rebuilt for since.
	mutable uint8_t* kbf = nullptr;
	mutable uint32_t* kbf_x = nullptr;
	mutable uint32_t kbf_fold = 0;
	mutable StaleRange kbf_stale;
	mutable void* mb = nullptr;
	mutable uint32_t* mb_n = nullptr;
	mutable uint32_t mb_pitch = 0;
	mutable std::vector<uint32_t> mb_n_host;
	// ranks mirror (msc_emd_ranks.hip): per slot the bins of its counted k-mers in bin order (rk_pitch entries, padded with 4^k) and
	// their number: the earth mover's distance of the Q x M pass in O(k-mers) instead of O(bins). Built from the digest mirror;
	// rk_stale: the slots written since
	mutable uint32_t* ranks = nullptr;
	mutable uint32_t* rk_n = nullptr;
	mutable uint64_t *rk_sum = nullptr, *rk_dev = nullptr;          // two moments per slot of that mirror (msc_emd_list.hip): one allocation, [capacity] each; null: none to be had
	mutable uint64_t rk_pitch = 0;
	mutable StaleRange rk_stale;
	mutable bool ranks_unavailable = false;
	// the ranges the cut of a folded block reads of its candidates (msc_fold_reject.h, MscRejectRanges: ten words on the device), over every slot the
	// mirrors have been built for; rj_stale: the slots written since (ensure_reject_ranges, msc_mirrors.hip). They only widen, until every slot is stale: then they start over
	mutable uint64_t* rj_ranges = nullptr;
	mutable StaleRange rj_stale;
	mutable uint64_t written_run = 0;          // dense sets: slots [0, written_run) are known to hold a histogram (reject_ranges_cover; `written` is never cleared)
	// ... and their 16-bit form (rank - floor(t * 4^k / pitch) + 32768; msc_emd_ranks.hip, k_emd_ranks16), kept while every slot's reduced
	// ranks fit and the pitch is a multiple of 1 024; rk16_off: a slot did not fit (or the allocation failed): the 32-bit walk stays
	mutable uint16_t* ranks16 = nullptr;
	mutable bool rk16_off = false;
	// sparse mirror of a DENSE set: the sorted (bin, value) lists of its slots, kept so that the divergence
	// statistics of every route come from the one merge kernel; sm_stale: the slots written since. Built on first use.
	mutable msc_hist_set* sp_mirror = nullptr;
	mutable StaleRange sm_stale;
	mutable bool sp_mirror_unavailable = false;
	std::vector<uint8_t> written;         // dense sets: slot holds a histogram (unwritten slots are never sparsified)
	// effective lengths as the host last learnt them (len_known[i] != 0): Trainer::get_close / filter / merge derive their length
	// window from the query's length, and reading it back from the device costs a stream round trip per call
	mutable std::vector<uint64_t> len_host;
	mutable std::vector<uint8_t> len_known;
	// sparse layout (sparse.hip): entry arena + per-slot headers instead of `bins`
	bool sparse = false;
	uint2* ent = nullptr;
	uint32_t* cum = nullptr;
	MscSparseHdr* hdr = nullptr;          // device, [capacity]
	std::vector<MscSparseHdr> hdr_host;   // mirror
	uint64_t ent_capacity = 0, ent_used = 0;
	uint32_t max_nnz = 0;                 // longest entry list ever stored (monotone)
	// rank lists of a sparse set (msc_ranks_pass.hip): per slot the bins of its counted k-mers, value - 1 copies of each, at rkl_off[slot],
	// rkl_n[slot] of them. A cache of the lists: every writer of a slot's list bumps list_epoch, the cache remembers the epoch it was built
	// at, and it is (re)built only once the same epoch has been asked for three times -- point sets build theirs once, centre stores (a
	// write every step) never do.
	uint64_t list_epoch = 0;
	mutable uint32_t* rkl = nullptr;
	mutable uint64_t* rkl_off = nullptr;
	mutable uint32_t* rkl_n = nullptr;
	mutable std::vector<uint64_t> rkl_off_host;          // (mirror: a pass whose query is a slot of this set reads its list in place)
	mutable uint64_t rkl_epoch = ~0ull, rkl_seen_epoch = ~0ull, rkl_entries = 0;
	mutable uint32_t rkl_seen = 0;
	mutable bool rkl_unavailable = false;
	// ... and beside them, for the long-list pass (k_pair_ranks_items), the slot's REPEATED bins: (bin, value - 1) for value >= 3, in bin
	// order, rkm_n[slot] of them at rkm_off[slot]; built at the first such pass of an epoch
	mutable uint2* rkm = nullptr;
	mutable uint64_t* rkm_off = nullptr;
	mutable uint32_t* rkm_n = nullptr;
	mutable uint64_t rkm_epoch = ~0ull, rkm_entries = 0;
};

struct msc_model {
	msc_ctx* ctx = nullptr;
	int k = 0;
	MscDevModel h;
	MscDevModel* d = nullptr;
	mutable bool fold_overflows = false;       // ... overflowed the list of their FOLDED stage (msc_fold.h): later calls run the true product
	mutable bool emd_decides = false;          // more than half the blocks of a msc_score_multi call overflowed the list of open pairs: later calls skip the bound pass (msc_emd_list.hip)
};


int fail(msc_ctx* ctx, int code, const char* fmt, ...);
extern const bool g_trace_calls;
#define HIP_TRY(ctx, expr)                                                                                 \
	do {                                                                                                   \
		if (g_trace_calls) { fprintf(stderr, "[msc] %s:%d %.160s\n", __FILE__, __LINE__, #expr); fflush(stderr); } \
		hipError_t e_ = (expr);                                                                            \
		if (g_trace_calls && e_ == hipSuccess) e_ = hipDeviceSynchronize();                                \
		if (e_ != hipSuccess)                                                                              \
			return fail(ctx, e_ == hipErrorOutOfMemory ? MSC_ERR_OOM : MSC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
			            hipGetErrorString(e_), __FILE__, __LINE__);                                        \
	} while (0)

int ensure(msc_ctx* ctx, DevBuf& b, size_t bytes);             // growable device scratch
int ensure_pinned(msc_ctx* ctx, DevBuf& b, size_t bytes);      // growable page-locked host staging
void release(DevBuf& b);
void mark_written(msc_hist_set* s, uint64_t first, uint64_t n);
// every writer of the lists of slots [first, first + n) of a sparse set ends here: the rank-list caches are keyed on list_epoch, the
// mirrors of the matrix-core pass (kb / mb / ranks, where the set has them) rebuild the stale range
void lists_written(msc_hist_set* s, uint64_t first, uint64_t n);
int refresh_bounds(msc_ctx* ctx, msc_hist_set* s, uint64_t first, uint64_t n);
void learn_length(const msc_hist_set* s, uint64_t slot, uint64_t len);
int slot_length(msc_ctx* ctx, const msc_hist_set* set, uint64_t slot, uint64_t* len);
int ensure_sparse_mirror(msc_ctx* ctx, const msc_hist_set* set, const msc_hist_set** out);

// the stages of the batched sparse mean (msc_api_batch.hip; msc_shard.hip puts an exchange between them)
int sparse_acc_prepare(msc_ctx* ctx, const MscLayout& L, uint32_t nc, uint32_t** touched_out);
int sparse_acc_scatter(msc_ctx* ctx, const msc_hist_set* src, const uint32_t* slots, const uint32_t* seg, uint64_t P, uint32_t* touched);
int sparse_acc_sweep(msc_ctx* ctx, const msc_hist_set* pts, uint32_t nc, const uint32_t* m_of, uint32_t* touched, uint64_t* floor_sum_out);
int sparse_distances_to_means(msc_ctx* ctx, const msc_hist_set* pts, const std::vector<MscBatchSeg>& segs, const std::vector<uint32_t>& pair_seg,
                              const std::vector<uint32_t>& members, uint32_t nc);
bool needs_wide(const msc_hist_set* a, const msc_hist_set* b);

// one 1 x M scoring pass (msc_api_score.hip): streaming kernel -> epilogue -> optional reduce
struct ScoreRequest {
	const msc_model* model = nullptr;
	const msc_hist_set* cands = nullptr;
	const uint32_t* cand_slots = nullptr;   // host
	uint64_t m = 0;
	const msc_hist_set* qset = nullptr;
	uint64_t q_slot = 0;
	int order = MSC_ORDER_CAND_FIRST;
	int use_window = 0;
	uint64_t min_len = 0, max_len = 0;
	uint64_t feat_mask = 0;
	// host outputs (nullable)
	double* raw_out = nullptr;
	double* singles_out = nullptr;
	double* combos_out = nullptr;
	double* sum_out = nullptr;
	double* csum_out = nullptr;
	double* combo0_out = nullptr;
	int32_t* status_out = nullptr;
	uint8_t* flags_out = nullptr;
	int reduce_mode = -1;                   // <0: no reduce kernel
	int64_t reduce_begin = 0;
	MscReduceOut* reduce_host = nullptr;
	bool only_tiles = false;                // msc_mean_nearest reuses the streaming kernel and folds partials itself
	bool slots_uploaded = false;            // ... and has put these very cand_slots into ctx->slots itself, on this stream (no second copy)
	// msc_get_close_window: the slot list is already on the device (cand_slots == nullptr), the close flags stay there, and
	// after_reduce queues its own kernel behind the reduce kernel, before the call's one stream sync (d_rec = the reduce record)
	const uint32_t* dev_slots = nullptr;
	uint8_t* dev_flags_out = nullptr;
	std::function<hipError_t(const MscReduceOut* d_rec)> after_reduce;
	// ... or, where the pass qualifies for the fused epilogue + reduce kernels, the window's close pass done inside them (pos != nullptr;
	// after_reduce is then not called)
	MscCloseList close_list{nullptr, nullptr, nullptr, nullptr};
};

int run_score(msc_ctx* ctx, ScoreRequest& rq);
