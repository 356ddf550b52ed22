// msc_api_private.h -- what the translation units of the C ABI's host side (msc_api.hip: context, sets, builds, models; msc_api_score.hip: the
// scoring driver and the 1 x M calls; msc_api_multi.hip: msc_score_multi; msc_mirrors.hip: the mirrors of a set the Q x M calls read; msc_api_batch.hip: the batched update stage; msc_api_pairlist.hip: msc_score_pair_list) share beyond
// msc_objects.h / msc_internal.h.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>

#include "msc_objects.h"
#include "msc_multi_plan.h"

// largest bin for which 32-bit per-lane partial sums of p*q cannot overflow: R * max^2 < 2^32 with R <= 64
static const uint64_t kNarrowMaxCount = 8191;
static const uint64_t kNarrowMaxSum = (1ull << 31) - 1;

// MSC_PROFILE_CALLS: the library's own timers inside a call (slot list / launches / stream wait), printed at msc_destroy
static const bool g_profile_calls = getenv("MSC_PROFILE_CALLS") != nullptr;
// from how many bins on the sparse mean sweeps only the 64-byte lines its members touched (MSC_SPARSE_MEAN_GROUPS_MIN_K for A/B runs; r05: from
// k = 9 on -- 200 000 x 1 kb: count + write sweeps 1.73 -> 0.38 ms per 4 150 centres, the update stage 1.27 -> 0.88 s; it was 11 only because the
// two places that cut a list into chunks disagreed below that)
static inline uint64_t msc_sparse_groups_min_bins() {
	static const uint64_t v = [] { const char* e = getenv("MSC_SPARSE_MEAN_GROUPS_MIN_K"); const int k = e ? atoi(e) : 9; return 1ull << (2 * std::max(5, std::min(16, k))); }();
	return v;
}
static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int check_slot(msc_ctx* ctx, const msc_hist_set* s, uint64_t slot);          // msc_api.hip: MSC_ERR_INVALID_ARG (with a message) for a slot outside the set

// ---- msc_api_score.hip
const uint64_t kSupportedFeats = MSC_FEAT_SLOW | MSC_FEAT_GROUPS;          // the statistics the GPU path evaluates
static inline double trainer_get_id(double cutoff) { return cutoff > 1 ? cutoff / 100.0 : cutoff; }      // cluster/Trainer.h:35
// both sets and the slots named exist and belong to ctx; same k and dtype
int validate_pair(msc_ctx* ctx, const msc_hist_set* cands, const msc_hist_set* qset, uint64_t q_slot, const uint32_t* slots, uint64_t m);
// the rule of the mirror pass: a DENSE set's passes may merge the lists of its sparse mirror -- not switched off (MSC_NO_SPARSE_MIRROR,
// msc_set_mirror_pass) and the histograms are not padded (the 1 x M calls and msc_score_pair_list)
bool mirror_pass_allowed(const msc_ctx* ctx, const MscLayout& L);
// the first failing pair's status as the call's: 0, or the status with the message of what the reference would have thrown
int pair_status(msc_ctx* ctx, int first_err);
// which of the merge kernels of sparse.hip takes a pass over the lists of c_sp against slot q_slot of q_sp
enum SparseKernel { SPK_LDS = 0, SPK_MP = 1, SPK_GENERIC = 2 };
SparseKernel pick_sparse_kernel(const msc_hist_set* c_sp, const msc_hist_set* q_sp, uint64_t q_slot, uint64_t max_count, bool wide);
// the rank lists of the sparse set (or sparse mirror) `s` (msc_ranks_pass.hip): true when they are current
bool rank_lists_ready(msc_ctx* ctx, const msc_hist_set* s, int* err, bool eager = false);
uint32_t sparse_records(SparseKernel k, uint32_t mp_parts = 1);          // records per candidate the merge kernel writes
uint32_t div_records(SparseKernel k, uint64_t entries);                  // ... and {jd, js} records per pair
// candidates [off, off + mc) (or the device slot list d_slots) of the sparse set / mirror c_sp against slot q_slot of q_sp
hipError_t launch_sparse_pass(msc_ctx* ctx, SparseKernel k, const msc_hist_set* c_sp, const uint8_t* c_scalars, uint64_t c_stride, const uint32_t* d_slots,
                              uint64_t off, uint32_t mc, const msc_hist_set* q_sp, uint64_t q_slot, const uint8_t* q_scal, uint64_t nbins, int use_window,
                              uint64_t min_len, uint64_t max_len, MscPartial* partials, void* div_tables, void* div_partials, int order, uint32_t parts = 1,
                              uint32_t div_stride = 1);

// ---- msc_api_batch.hip (shared with msc_api_pairlist.hip): the two divergence sums of a pair list
// which lists to merge (the sets themselves, or the sparse mirrors of dense sets); *ok = false when a 1 x M call on these sets would not take the
// chunked merge kernel -- the caller then goes query by query
int batch_div_lists(msc_ctx* ctx, const msc_hist_set* cands, const msc_hist_set* queries, uint64_t any_q_slot, const msc_hist_set** c_sp, const msc_hist_set** q_sp, bool* ok);
// the pass, for P pairs described by ctx->slots / ctx->segs / ctx->pair_seg: sums -> ctx->div_partials[pair][*div_n][2], integer records -> partials
int batch_div_pass(msc_ctx* ctx, const msc_hist_set* cands, const msc_hist_set* queries, const msc_hist_set* c_sp, const msc_hist_set* q_sp, uint64_t P, int order,
                   MscPartial* partials, uint32_t* div_n);

// ---- msc_mirrors.hip: the mirrors of a set that the Q x M calls read (msc_api_multi.hip, msc_api_pairs.hip), each built on first use
int ensure_digest(msc_ctx* ctx, const msc_hist_set* set);      // the digest mirror of a dense set (set->digest null: unavailable)
int ensure_kb(msc_ctx* ctx, const msc_hist_set* set, bool want_fold = false);          // the presence-bit mirror and lists of large bins of a set, from its bins or its lists (set->kb null: unavailable); want_fold: and its folded form
int ensure_ranks(msc_ctx* ctx, const msc_hist_set* set);       // the ranks mirror, likewise (set->ranks null: unavailable)
int ensure_reject_ranges(msc_ctx* ctx, const msc_hist_set* set);          // the ranges of the slots' scalars, moments and lists behind the cut of a folded block (set->rj_ranges null: unavailable)
bool reject_ranges_cover(const msc_hist_set* set, const uint32_t* slots, uint64_t m);          // ... and whether they cover the m candidates of a call
bool kb_route_fits(const msc_hist_set* cands, const msc_hist_set* qset, bool need_emd);          // host-side bounds of the matrix-core pass
void mark_stale(msc_hist_set* s, uint64_t first, uint64_t n);  // slots [first, first + n) were written: the mirrors the set has are stale there
void free_mirrors(const msc_hist_set* set);                    // msc_hist_set_destroy
uint64_t mirror_bytes_per_slot(const msc_hist_set* s);         // the mirrors' term of msc_hist_set_bytes

// ---- msc_api_multi.hip (shared with msc_api_pairs.hip)
int read_error_word(msc_ctx* ctx);                             // the epilogue's error word as a status (the stream is idle)
// ... and what a block on the matrix cores needs in either driver (the drivers themselves stay apart: msc_score_multi pipes its blocks over three
// streams and scores every pair, msc_search_pairs lists the close ones on one stream)
uint64_t block_hot_size(const msc_hist_set* qset, const uint32_t* q_slots, uint64_t nq);          // entries of the hot list of a block of query slots
// the candidate chunks of a block of `rows` query rows: the product array [slices][chunk][rows] int32 within 2 GiB, at most `limit` candidates a chunk
MscCandChunks matrix_chunks(const msc_ctx* ctx, uint64_t nbins, uint64_t m, uint32_t rows, uint64_t limit = ~0ull);
struct HotList { uint32_t *ptr = nullptr, *cursor = nullptr, *cnt = nullptr; };          // the three step arrays of a hot list (null: the list is empty)
int ensure_side(msc_ctx* ctx, BlockPipe::Side& s, uint64_t nbins, uint32_t rows, uint32_t slices, uint64_t chunk, uint64_t n_hot, HotList* hot);
// the epilogue's arguments cleared, then the fields that say which pairs a chunk holds: nq queries (device slots dq, the first one's host slot q_slot0)
// x mc candidates (device slot list d_slots, or slots from `first` on), n_rec records per pair
void fill_pair_args(MscEpilogueArgs& ea, msc_ctx* ctx, const msc_hist_set* cands, const msc_hist_set* qset, const uint32_t* d_slots, uint64_t first, uint32_t mc, const uint32_t* dq, uint32_t q_slot0, uint32_t nq, uint32_t n_rec, int order);
// the kb_* and emd_* fields of the epilogue's arguments (first: the chunk's first candidate, 0 with a slot list; emd_out null: no emd)
void fill_matrix_args(MscEpilogueArgs& ea, const BlockPipe::Side& s, const msc_hist_set* cands, const msc_hist_set* qset, uint32_t slices, uint32_t rows, uint64_t first, uint64_t n_hot, const void* emd_out);
// the earth mover's distances of a chunk from the ranks mirrors: the 16-bit walk where both sets keep that form at one pitch
hipError_t launch_emd_ranks(hipStream_t st, const msc_hist_set* cands, const msc_hist_set* qset, const uint32_t* d_slots, uint64_t off, uint32_t mc, const uint32_t* dq, uint32_t nq, uint64_t* out, uint32_t stride, const uint32_t* run_if = nullptr);
void name_matrix_kernel(msc_ctx* ctx, uint32_t rows, bool emd, bool cells, bool from_lists, uint32_t fold = 0);      // msc_last_kernel_info's name of the product kernel
