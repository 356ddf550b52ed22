// msc_internal.h -- declarations shared between the C-ABI translation unit and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/meshclust2_hip.h"
#include "msc_layout.h"

// ---------------------------------------------------------------- sparse slots (sparse.hip)
#define MSC_SPARSE_SUB 16
struct MscSparseHdr {
	uint64_t off;                       // first entry of this slot in the set's entry arena
	uint32_t nnz;                       // entries (bins with value >= 2)
	uint32_t split[MSC_SPARSE_SUB + 1]; // entry offsets (relative to off) of the 16 equal index sub-ranges; split[16] == nnz
	uint32_t pad_[2];
};
static_assert(sizeof(MscSparseHdr) == 88, "sparse header layout");

// ---------------------------------------------------------------- model, as the epilogue kernel sees it
struct MscDevModel {
	int32_t  n_singles;
	int32_t  n_combos;
	uint64_t single_flag[MSC_MAX_SINGLES];
	double   mins[MSC_MAX_SINGLES];
	double   maxs[MSC_MAX_SINGLES];
	int32_t  is_sim[MSC_MAX_SINGLES];
	int32_t  combo_kind[MSC_MAX_COMBOS];
	int32_t  combo_n[MSC_MAX_COMBOS];
	int32_t  combo_idx[MSC_MAX_COMBOS][2];
	double   weights[MSC_MAX_COMBOS + 1];
	double   bias;
	// f32 image of the same model for the close-flag screen of k_pair_epilogue_bits (pair_features.hip, screen_close): filled by
	// msc_model_create; screen_ok = 0 when the model is outside what the screen bounds (a statistic that is not an integer reduction,
	// a bias, a non-finite constant)
	int32_t  screen_ok;
	float    s_min[MSC_MAX_SINGLES];          // mins[i]
	float    s_inv[MSC_MAX_SINGLES];          // 1 / (maxs[i] - mins[i])
	float    s_w[MSC_MAX_COMBOS + 1];         // weights
};

// One 1 x M problem of a batched launch (k_pair_tiles_batch, k_colsum_batch): query slot, its candidates' positions in the
// concatenated slot list, and the length window of Trainer::filter (ignored when the launch does not use a window).
struct MscBatchSeg {
	uint32_t q_slot, first, m, pad_;
	uint64_t min_len, max_len;
};

// One partial record per (candidate, tile): integer reductions of the streaming pass.
struct MscPartial {
	uint64_t manh;   // sum |p - q|
	uint64_t dot;    // sum p * q
	uint64_t emd;    // sum |prefix(p) - prefix(q)|
};

// Per-candidate result of the epilogue kernel.
struct MscPairOut {
	double  sum;       // weighted sum s
	double  csum;      // logistic(s) + bias
	double  combo0;    // first combo ("similarity" used for the arg-max)
	int32_t status;    // 0 ok, 1 skipped by the length window, MSC_ERR_* (negative) if the reference would throw
	int32_t close;     // round(csum) > 0
};

struct MscReduceOut {
	double  best_sim;
	int64_t best_pos;
	int32_t any_close;
	int32_t first_error;   // most negative status seen (0 if none)
	uint64_t n_close;
};

enum { MSC_REDUCE_GET_CLOSE = 0, MSC_REDUCE_MERGE = 1 };

// epilogue request
struct MscEpilogueArgs {
	const MscPartial* partials;       // [m][S]
	const void* partials16;           // or: [m][S] records of four u32 {manh, dot, emd, 0} (ring kernel); partials is then unused
	const void* partials_cq;          // or: [m_per_query][ceil(n_queries/16)][S][16] such records (digest kernel: one 256-byte run per workgroup step)
	uint32_t cq_group;                // with partials_cq: queries per group -- 16, or 32 with 4-byte records (manh only: dot_gemm set, emd from emd_ranks or not wanted)
	const uint64_t* emd_ranks;        // with partials_cq: the earth mover's distances from msc_emd_ranks.hip instead, [m_per_query][64] (query q at [q])
	const int32_t* dot_gemm;          // with partials_cq: the products from msc_dot_gemm.hip instead, [dot_slices][m_per_query][dot_stride] (query q at [q]);
	                                  // the records of partials_cq are then 8 bytes (manh, emd)
	uint32_t dot_slices, dot_stride;
	// the r04 pass on the matrix cores (msc_pair_gemm.hip, k_pair_epilogue_bits): P1 per slice and P2 of the block, the lists of large
	// bins (e = count - 1 >= 2) of both sets, the queries' counts [bin][kb_qn] (bytes, clamped at 127)
	const int32_t* kb_min;            // [kb_slices][m_per_query][kb_qn]; non-null selects k_pair_epilogue_bits
	const int32_t* kb_diff;           // [m_per_query][kb_qn], or null when no query of the block has a large bin
	uint32_t kb_slices, kb_qn;
	uint64_t kb_first;                // slot of candidate 0 when cand_slots is null (cand_scalars is then already offset to it)
	const void* kb_c_mb;              // uint2 (bin, e) [slot][kb_c_pitch]
	const uint32_t* kb_c_mb_n;
	uint32_t kb_c_pitch;
	const void* kb_q_mb;
	const uint32_t* kb_q_mb_n;
	uint32_t kb_q_pitch;
	const uint8_t* kb_qT;
	uint32_t emd_stride;              // entries per candidate of emd_ranks (0 = 64)
	const void* div_partials;         // [m][S] {jd, js} doubles, or null when no divergence statistic is requested
	uint32_t S;
	uint32_t m;
	const uint8_t* cand_scalars;      // scalar records of the candidate set
	uint64_t cand_scalar_stride;
	const uint32_t* cand_slots;       // nullable -> identity
	const uint8_t* q_scalars;         // scalar record of the query (already offset to its slot)
	// several queries in one launch (virtual candidate index = qi * m_per_query + ci); n_queries <= 1 -> q_scalars above
	uint32_t n_queries, m_per_query;
	const uint32_t* q_slots;          // device, [n_queries]
	const uint8_t* qset_scalars;
	uint64_t q_scalar_stride;
	uint64_t nbins;
	int32_t  dtype;
	int32_t  order;                   // MSC_ORDER_*
	int32_t  use_window;              // skip candidates outside [min_len, max_len]
	uint64_t min_len, max_len;
	// raw feature output
	uint64_t feat_mask;               // bits to emit in ascending order
	double*  raw_out;                 // [m][popcount(feat_mask)] or null
	// model output
	const MscDevModel* model;         // device pointer or null
	double*  singles_out;             // [m][n_singles] or null
	double*  combos_out;              // [m][n_combos] or null
	MscPairOut* pair_out;             // [m] or null
	// structure-of-arrays outputs (device, nullable): what the all-pairs path copies back instead of pair_out
	double*  sum_soa;
	double*  csum_soa;
	uint8_t* close_soa;
	int32_t  screen;                  // k_pair_epilogue_bits: only close_soa is wanted and the model has an f32 image -- decide in f32 with an error bound, FP64 where that does not decide
	int32_t* error_word;              // atomicMin of negative statuses
	// batched launch (k_pair_tiles_batch): candidate c belongs to segment pair_seg[c]; query slot and window come from it
	const MscBatchSeg* segs;
	const uint32_t* pair_seg;
	uint64_t sparse_base;             // 4^k when the partials come from k_pair_sparse (sums over the union only), else 0
	// divergence statistics from the sparse merge kernels (sparse sets, and dense sets through their sparse mirror): per pair
	// div_direct_n records of {jd, js} summed over the union of stored bins, relative to the (1, 1) term; div_base = 4^k adds it back
	const double* div_direct;         // [pairs][div_direct_n][2], pair index = the virtual candidate index
	uint32_t div_direct_n;
	uint64_t div_base;
	// statistics over 4-bin groups (sim_mm through markov, rre_k_r; k_pair_sparse_groups / k_sparse_self_markov): 16 partial
	// records per pair / per histogram, summed in sub-range order by the epilogue
	const double* grp_pairs;          // [pairs][16][2] = {markov, rre}
	const double* grp_self_c;         // [m_per_query or m][16]: markov(c, c) of every candidate of the launch (index = candidate position)
	const double* grp_self_q;         // [n_queries or 1][16]: markov(q, q)
	// msc_search_pairs with msc_set_pairs_div_cells, msc_score_multi with msc_set_multi_div_cells: the divergence statistics on the matrix-core
	// route, from (count, count) cells and the two lists of large bins (k_pair_epilogue_bits_div -- through msc_launch_epilogue for
	// msc_score_multi --, k_pair_list_write<true, true>); kb_c_bits = the candidates' presence mirror
	const uint8_t* kb_c_bits;
	int32_t  div_cells;
	// msc_score_multi's close flags without the dense rank walk (msc_emd_list.hip; k_pair_epilogue_bits_bound / _list): the two moments per slot of both
	// sets' ranks mirrors, the list of the pairs the bounds leave open (pair index q * m_per_query + ci), its words {count, overflow}, its capacity,
	// and the exact distances of the listed pairs
	const uint64_t *rk_c_sum, *rk_c_dev, *rk_q_sum, *rk_q_dev;
	uint32_t* open_list;
	uint32_t* open_words;
	uint32_t open_cap;
	const uint64_t* emd_list;
	// k_pair_epilogue_bits_screen / _open: null, or a device word -- the launch does nothing when it is 0 (queued behind the list kernels for the case
	// that the list overflowed)
	const uint32_t* run_if;
	// k_pair_epilogue_bits_bound on a FOLDED block (msc_fold.h): kb_min / kb_diff then hold P1' / P2' of the folded product, upper bounds of P1 / P2
	// with each slot's own collisions added (fold_x_c: by candidate slot, fold_x_q: by query slot); null: the product was exact
	const uint32_t *fold_x_c, *fold_x_q;
	// ... and the integer cut of its rows (msc_fold_reject.h, k_fold_reject_cut): fold_cut[q] = T(q), or negative: none. A candidate whose P1' + P2' is at most
	// the cut in every lane of a wave is "not close" without an evaluation. fold_cut_words[0] counts the pairs evaluated in rows that have a cut. null: no cuts
	const int32_t* fold_cut;
	unsigned long long* fold_cut_words;
	// k_pair_epilogue_bits_bound / _list over a GROUP of blocks of 128 query rows (msc_tail_groups, msc_multi_plan.h): blockIdx.y is the block of the group,
	// and its kb_min, kb_diff, kb_qT, close_soa (bytes), q_slots, open_list and emd_list (entries), open_words (words) lie that many strides behind the
	// first block's; tg_blocks is their number, the launch's gridDim.y. All 0: a launch over one block
	uint64_t tg_min_stride, tg_diff_stride, tg_qt_stride, tg_flags_stride, tg_list_stride;
	uint32_t tg_q_stride, tg_words_stride, tg_blocks;
};

// ---------------------------------------------------------------- launchers (defined in the .hip kernel files)
// f(T{}) for the bin type T of `dtype` bits (8, 16, 32, otherwise 64); returns what f returns
template <typename F>
static inline auto msc_by_dtype(int dtype, F&& f) {
	switch (dtype) {
	case 8: return f(uint8_t{});
	case 16: return f(uint16_t{});
	case 32: return f(uint32_t{});
	default: return f(uint64_t{});
	}
}

hipError_t msc_launch_fill(hipStream_t st, void* bins, const MscLayout& L, uint64_t first_slot, uint64_t n_slots);
hipError_t msc_launch_count(hipStream_t st, void* bins, uint8_t* scalars, const MscLayout& L, int k, int dtype,
                            uint64_t first_slot, const uint32_t* packed_words, const uint32_t* seg_seq,
                            const uint64_t* seg_start, const uint64_t* kmer_off, uint64_t n_segs,
                            uint64_t total_kmers, bool saturating);
hipError_t msc_launch_finalize(hipStream_t st, const void* bins, uint8_t* scalars, const MscLayout& L, int dtype,
                               uint64_t first_slot, uint64_t n_slots, bool keep_mag, uint64_t* tile_scratch = nullptr);
bool msc_lds_build_supported(const MscLayout& L);
bool msc_sort_build_supported(const MscLayout& L, int k);
uint32_t msc_sort_build_max_kmers();
hipError_t msc_launch_build_sort(hipStream_t st, void* bins, uint8_t* scalars, const MscLayout& L, int k, int dtype, uint64_t first_slot,
                                 const uint32_t* seq_ids, uint64_t n, uint32_t P, const uint32_t* packed_words, const uint64_t* seg_start,
                                 const uint64_t* kmer_off, const uint64_t* seq_seg_begin, const uint64_t* seq_meta, uint64_t* bounds);
hipError_t msc_launch_build_lds(hipStream_t st, void* bins, uint8_t* scalars, const MscLayout& L, int k, int dtype, uint64_t first_slot,
                                uint64_t n_seqs, const uint32_t* packed_words, const uint64_t* seg_start, const uint64_t* kmer_off,
                                const uint64_t* seq_seg_begin);
hipError_t msc_launch_permute(hipStream_t st, const void* src, void* dst, const MscLayout& L, int dtype, bool to_physical);

hipError_t msc_launch_pair_tiles(hipStream_t st, const MscLayout& L, int dtype,
                                 const uint8_t* cand_bins, const uint8_t* cand_scalars, const uint32_t* cand_slots,
                                 uint32_t m, const uint8_t* q_bins_slot, const uint8_t* q_scalars_slot,
                                 int use_window, uint64_t min_len, uint64_t max_len, MscPartial* partials,
                                 int num_cus, void* div_tables /*nullable*/, void* div_partials, int order);
hipError_t msc_launch_pair_tiles_multi(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* cand_bins, const uint8_t* cand_scalars,
                                       const uint32_t* cand_slots, uint32_t m, const uint8_t* qset_bins, uint64_t q_slot_bytes,
                                       const uint8_t* qset_scalars, uint64_t q_scalar_stride, const uint32_t* q_slots, uint32_t n_q,
                                       int tq, bool compact, MscPartial* partials, int num_cus);
hipError_t msc_launch_pair_tiles_wide(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* cand_bins, const uint8_t* cand_scalars,
                                      const uint32_t* cand_slots, uint32_t m, const uint8_t* q_bins_slot, const uint8_t* q_scalars_slot,
                                      int use_window, uint64_t min_len, uint64_t max_len, MscPartial* partials, int num_cus,
                                      void* div_partials /*nullable*/, int order);
int msc_div_table_dim(const MscLayout& L);      // 8 or 16: side of the per-candidate (count, count) term table
// Q x M streaming through the LDS-DMA ring (32/64-bit bins, LPT 4, compact totals, tq 4 or 8). hipErrorInvalidValue = not applicable.
hipError_t msc_launch_pair_tiles_multi_ring(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* cand_bins, const uint8_t* cand_scalars,
                                            const uint32_t* cand_slots, uint32_t m, const uint8_t* qset_bins, uint64_t q_slot_bytes,
                                            const uint8_t* qset_scalars, uint64_t q_scalar_stride, const uint32_t* q_slots, uint32_t n_q, int tq,
                                            bool prefix16, void* partials16, int num_cus);
// digest mirror of an 8/16/32-bit set (pair_digest.hip): 4 bytes per bin whatever the bin type; build for slots [first, first+n),
// and the Q x M pass that streams it
bool msc_digest_supported(const MscLayout& L);
uint64_t msc_digest_slot_bytes(const MscLayout& L);
hipError_t msc_launch_digest_build(hipStream_t st, const MscLayout& L, const uint8_t* bins, const uint8_t* scalars, uint8_t* digest, uint64_t first_slot,
                                   uint64_t n_slots);
int msc_digest_tiles_per_step(const MscLayout& L, uint64_t max_count);      // 1 or 2 consecutive tiles scored per loop step
hipError_t msc_launch_pair_digest_multi(hipStream_t st, const MscLayout& L, const uint8_t* cand_digest, const uint32_t* cand_slots, uint32_t m,
                                        const uint8_t* q_digest, const uint32_t* q_slots, uint32_t n_q, bool counts_fit_u8,
                                        int tiles_per_step, bool need_emd, void* partials16, int num_cus, bool need_dot = true, int queries_per_wave = 4);
// the products of the Q x M pass as an int8 GEMM on the matrix cores (msc_dot_gemm.hip)
uint64_t msc_ranks_pitch(uint64_t max_excess);
hipError_t msc_launch_ranks_build(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* bins, const uint8_t* scalars, uint32_t* ranks, uint32_t* n_of, uint64_t pitch,
                                  uint64_t first_slot, uint64_t n_slots, int32_t* bad);
hipError_t msc_launch_ranks_build_sparse(hipStream_t st, const MscLayout& L, const void* ent, const uint32_t* cum, const MscSparseHdr* hdr, uint32_t* ranks, uint32_t* n_of,
                                         uint64_t pitch, uint64_t first_slot, uint64_t n_slots, int32_t* bad);
hipError_t msc_launch_emd_ranks(hipStream_t st, uint64_t nbins, const uint32_t* c_ranks, uint64_t c_pitch, const uint32_t* c_n, const uint32_t* cand_slots, uint64_t first,
                                uint32_t m, const uint32_t* q_ranks, uint64_t q_pitch, const uint32_t* q_n, const uint32_t* q_slots_dev, uint32_t n_q, uint64_t* out,
                                uint32_t out_stride = 64, const uint32_t* run_if = nullptr);
hipError_t msc_launch_ranks16_build(hipStream_t st, uint64_t nbins, const uint32_t* ranks, uint16_t* ranks16, uint64_t pitch, uint64_t first_slot, uint64_t n_slots, int32_t* bad);
hipError_t msc_launch_emd_ranks16(hipStream_t st, uint64_t nbins, const uint16_t* c_ranks, uint64_t pitch, const uint32_t* c_n, const uint32_t* cand_slots, uint64_t first,
                                  uint32_t m, const uint16_t* q_ranks, const uint32_t* q_n, const uint32_t* q_slots_dev, uint32_t n_q, uint64_t* out, uint32_t out_stride, const uint32_t* run_if = nullptr);
// msc_emd_list.hip: two moments per slot of the ranks mirror that bound the distance of a pair, the exact distances of a device list of pairs, and the
// bookkeeping of that list (words = {pairs appended, overflow}; totals = {pairs walked, blocks that overflowed} of a call)
hipError_t msc_launch_rank_moments(hipStream_t st, uint64_t nbins, const uint32_t* ranks, uint64_t pitch, uint64_t first_slot, uint64_t n_slots, uint64_t* rk_sum, uint64_t* rk_dev);
// The list kernels over a GROUP of blocks of 128 query rows (msc_tail_groups, msc_multi_plan.h): blockIdx.y is the block of the group, whose query slots, list,
// emd_list (entries), words, transposed planes, P1 and P2 (bytes) lie that many strides behind the first block's. The grid is sized for the group's
// total capacity. n_blocks 0 or 1 with every stride 0: a launch over one block
struct MscListGroup { uint32_t n_blocks, q_stride, words_stride; uint64_t list_stride, qt_stride, min_stride, diff_stride; };
hipError_t msc_launch_emd_ranks_list(hipStream_t st, bool u16, const void* c_ranks, const void* q_ranks, uint64_t pitch, const uint32_t* cand_slots, uint64_t first, uint32_t m_per_query,
                                     const uint32_t* q_slots_dev, const uint32_t* list, const uint32_t* words, uint32_t cap, uint64_t* emd_list, int num_cus,
                                     const MscListGroup* grp = nullptr);
// (fold_flag: null, or the word of a FOLDED block: set when its list overflowed, which totals[2] counts instead of totals[1])
// n_blocks > 1: the lists of a group's blocks, closed in block order in one launch -- block j's words at words + j * words_stride, its flag at fold_flag + j
hipError_t msc_launch_emd_list_close(hipStream_t st, uint32_t* words, uint32_t cap, uint64_t* totals, uint32_t* fold_flag = nullptr, uint32_t n_blocks = 1, uint32_t words_stride = 0);
// the exact P1 / P2 of the listed pairs of a folded block, from the candidate's row of the 32-bit ranks mirror and the queries' transposed planes
struct MscFoldExact {
	const uint32_t* c_ranks; uint64_t pitch; uint64_t nbins; uint32_t E, R;
	const uint32_t* cand_slots; uint64_t first; uint32_t m_per_query;
	const uint32_t* q_slots; const uint32_t* list; const uint32_t* words; uint32_t cap;
	const uint8_t* qT; uint32_t qn;
	const void* q_mb; const uint32_t* q_mb_n; uint32_t q_pitch;
	int32_t* out_min; uint32_t slices; int32_t* out_diff;
};
hipError_t msc_launch_fold_exact_list(hipStream_t st, const MscFoldExact& a, int num_cus, const MscListGroup* grp = nullptr);
// msc_fold_reject.hip: the ranges of a set's slots the cut's certificate reads (ten words in the order of MscRejectRanges, msc_fold_reject.h: atomic min / max
// into what they hold), and the cut of every query row of a block or of a tail group's blocks: out[0 .. n_out), rows past n_rows without a cut;
// words[1] += the rows without a cut (null: not counted)
hipError_t msc_launch_fold_reject_ranges(hipStream_t st, const uint8_t* scalars, uint64_t scalar_stride, const void* mb, const uint32_t* mb_n, uint32_t pitch, const uint64_t* rk_dev,
                                         uint64_t first, uint64_t n, uint64_t* ranges);
struct MscFoldRejectCut {
	const MscDevModel* model; const uint64_t* ranges; uint64_t nbins; int32_t dtype, order;
	const uint32_t* q_slots; uint32_t n_rows, n_out;
	const uint8_t* q_scalars; uint64_t q_scalar_stride; const uint64_t* q_rk_dev; const uint32_t* q_x;
	const void* q_mb; const uint32_t* q_mb_n; uint32_t q_pitch;
	int32_t* out; unsigned long long* words;
};
hipError_t msc_launch_fold_reject_cut(hipStream_t st, const MscFoldRejectCut& a);
// the r04 form of that pass (msc_pair_gemm.hip): presence-bit mirror + lists of large bins, the queries' side of a block, the product
uint64_t msc_kb_bytes(const MscLayout& L, uint64_t capacity);
hipError_t msc_launch_kb_build(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* bins, uint8_t* kb, uint64_t first_slot, uint64_t n_slots, void* mb,
                               uint32_t* mb_n, uint32_t pitch, int32_t* flags);
bool msc_kb_build_sparse_fits(const MscLayout& L);
hipError_t msc_launch_kb_build_sparse(hipStream_t st, const MscLayout& L, const void* ent, const MscSparseHdr* hdr, uint8_t* kb, uint64_t first_slot, uint64_t n_slots,
                                      void* mb, uint32_t* mb_n, uint32_t pitch, int32_t* flags);
uint32_t msc_pair_gemm_rows(uint32_t n_q);
// msc_ranks_pass.hip: the 1 x M pass over rank lists
size_t msc_ranks_pass_lds(uint64_t nbins, uint64_t q_kmers);
uint32_t msc_ranks_pass_query_cap();
hipError_t msc_launch_rank_lists_sizes(hipStream_t st, const MscSparseHdr* hdr, const uint32_t* cum, uint64_t capacity, uint32_t* n, uint64_t* off);
hipError_t msc_launch_rank_lists_fill(hipStream_t st, const void* ent, const uint32_t* cum, const MscSparseHdr* hdr, uint64_t capacity, const uint32_t* n, const uint64_t* off,
                                      uint64_t nbins, uint32_t* out);
// the divergence statistics of a long-list rank pass (msc_ranks_pass.hip): what the launch needs beside its own scratch
struct MscRankDiv {
	uint32_t* big;              // [the query's stored bins] the counts >= 8
	const uint8_t* q_scalars;   // the query's scalar record
	int order;
	double* div_out;            // [m][2] the {jd, js} record of each candidate
};
hipError_t msc_launch_pair_ranks_1xm(hipStream_t st, const uint32_t* c_rk, const uint64_t* c_off, const uint32_t* c_n, const uint8_t* cand_scalars, uint64_t scalar_stride,
                                     const uint32_t* cand_slots, uint64_t first, uint32_t m, const void* q_ent, const uint32_t* q_cum, const MscSparseHdr* q_hdr, uint64_t nbins,
                                     int use_window, uint64_t min_len, uint64_t max_len, MscPartial* partials, int num_cus, uint64_t q_kmers, uint32_t* guard, uint32_t* q_scratch);
uint64_t msc_ranks_pass_query_scratch(uint64_t q_kmers);
uint32_t msc_ranks_items_round();
size_t msc_ranks_items_rec_bytes(uint64_t m, uint32_t rounds);                   // the pass's records and spot-term slots, one per item
size_t msc_ranks_items_list_bytes(uint64_t m, uint32_t rounds);                  // ... its candidates' records and its list of items
hipError_t msc_launch_pair_ranks_items(hipStream_t st, const uint32_t* c_rk, const uint64_t* c_off, const uint32_t* c_n, const void* c_rm, const uint64_t* c_rm_off,
                                       const uint32_t* c_rm_n, const uint8_t* cand_scalars, uint64_t scalar_stride, const uint32_t* cand_slots, uint64_t first, uint32_t m,
                                       const void* q_ent, const uint32_t* q_cum, const MscSparseHdr* q_hdr, uint64_t nbins, int use_window, uint64_t min_len, uint64_t max_len,
                                       MscPartial* partials, int num_cus, uint32_t* q_scratch, uint32_t rounds, void* rec_scratch, const MscRankDiv* dv, uint64_t q_kmers,
                                       uint32_t* guard, void* item_scratch, uint32_t* counters, uint32_t* tables, int turn, const uint32_t* q_rk);
uint32_t msc_ranks_items_table_words(uint64_t nbins);
// the repeated-bin lists of a sparse set (bin, count - 1 for the bins counted twice and more), beside its rank lists
hipError_t msc_launch_rank_multi_sizes(hipStream_t st, const void* ent, const MscSparseHdr* hdr, uint64_t capacity, uint32_t* n, uint64_t* off);
hipError_t msc_launch_rank_multi_fill(hipStream_t st, const void* ent, const MscSparseHdr* hdr, uint64_t capacity, const uint64_t* off, void* out);
const char* msc_pair_gemm_kernel_name();          // "k_pair_gemm_fp4_dma"
uint32_t msc_pair_gemm_slices(uint64_t nbins, uint32_t m, uint32_t qn, int num_cus);
uint64_t msc_pair_gemm_qt_bytes(uint64_t nbins, uint32_t qn);
uint64_t msc_pair_gemm_anib_bytes(uint64_t nbins, uint32_t qn);          // the queries' nibble tiles for the LDS-DMA form of the product (0: off)
hipError_t msc_launch_pair_gemm_queries(hipStream_t st, uint64_t nbins, const uint8_t* q_kb, const void* q_mb, const uint32_t* q_mb_n, uint32_t q_pitch,
                                        const uint32_t* q_slots_dev, uint32_t n_q, uint32_t qn, uint8_t* qT, uint64_t n_hot, void* hot, uint32_t* hot_ptr,
                                        uint32_t* hot_cursor, uint32_t* hot_cnt, uint8_t* anib);
hipError_t msc_launch_pair_gemm(hipStream_t st, uint64_t nbins, const uint8_t* cand_kb, const uint32_t* cand_slots, uint64_t first, uint32_t m, uint32_t qn,
                                uint32_t k_slices, const uint32_t* hot_ptr, const void* hot, int32_t* out_min, int32_t* out_diff, const uint8_t* anib, bool diff_zeroed = false);
// the folded mirror of a set (msc_fold.h) and the two parts of the queries' side on their own
hipError_t msc_launch_kb_fold(hipStream_t st, uint64_t nbins, uint32_t fold, const uint8_t* kb, uint8_t* kbf, uint32_t* x, uint64_t first_slot, uint64_t n_slots);
hipError_t msc_launch_kb_gather(hipStream_t st, uint64_t nbins, const uint8_t* q_kb, const uint32_t* q_slots_dev, uint32_t n_q, uint32_t qn, uint8_t* qT, uint8_t* anib);
hipError_t msc_launch_hot_list(hipStream_t st, uint64_t nbins, uint32_t fold, const void* q_mb, const uint32_t* q_mb_n, uint32_t q_pitch, const uint32_t* q_slots_dev,
                               uint32_t n_q, uint32_t qn, uint8_t* qT, uint64_t n_hot, void* hot, uint32_t* hot_ptr, uint32_t* hot_cursor, uint32_t* hot_cnt);
// ... and both parts for a group of blocks of 128 rows in one set of launches (msc_query_groups, msc_multi_plan.h): images and lists a stride apart
hipError_t msc_launch_query_group(hipStream_t st, uint64_t nbins, uint32_t fold, const uint8_t* q_kb, const uint8_t* q_kbf, const void* q_mb, const uint32_t* q_mb_n,
                                  uint32_t q_pitch, const uint32_t* q_slots_dev, uint32_t n_blocks, uint32_t n_q_last, uint8_t* qT, uint64_t qt_stride, uint8_t* anib,
                                  uint64_t anib_stride, uint64_t hot_stride, void* hot, uint32_t* hot_ptr, uint32_t* hot_cursor, uint32_t* hot_cnt, uint64_t idx_stride);
hipError_t msc_launch_epilogue(hipStream_t st, const MscEpilogueArgs& a);
hipError_t msc_launch_epilogue_bound(hipStream_t st, const MscEpilogueArgs& a);
hipError_t msc_launch_epilogue_list(hipStream_t st, const MscEpilogueArgs& a, int num_cus);
hipError_t msc_launch_close_counts(hipStream_t st, const uint8_t* flags, uint32_t n_q, uint32_t m, uint64_t* counts);
// the list of close pairs of msc_search_pairs (pair_features.hip): records of (query, tile of candidates), counted, scanned, written
uint32_t msc_pair_list_tiles(uint32_t mc);
hipError_t msc_launch_pair_list_flags(hipStream_t st, const MscEpilogueArgs& a, unsigned long long* open);
hipError_t msc_launch_pair_list_count(hipStream_t st, const uint8_t* flags, uint32_t n_q, uint32_t mc, uint64_t first, const uint64_t* win_lo, const uint64_t* win_hi,
                                      uint32_t* counts);
hipError_t msc_launch_pair_list_scan(hipStream_t st, const uint32_t* counts, uint32_t n_q, uint32_t tiles, uint64_t* base, uint64_t* offsets, uint64_t* qcount, uint64_t* seg);
hipError_t msc_launch_pair_list_write(hipStream_t st, const MscEpilogueArgs& a, const uint8_t* flags, uint64_t first, const uint64_t* win_lo, const uint64_t* win_hi,
                                      const uint64_t* offsets, uint32_t* out_idx, double* out_sim);
hipError_t msc_launch_pair_list_gather(hipStream_t st, const uint64_t* seg, uint32_t n_chunks, uint32_t n_q, uint64_t* base, uint64_t* dst, const uint32_t* s_idx,
                                       const double* s_sim, uint32_t* out_idx, double* out_sim);
// the merge of msc_search_pairs_strands: the lists F and R of one call (offsets off_f / off_r per query, ascending candidate index inside a query) into
// their union per query. count: r_only[entry of R] and counts[q], scanned into off_m[0 .. n_q]; write: the merged list with a strand byte per pair
hipError_t msc_launch_pair_strand_count(hipStream_t st, const uint64_t* off_f, const uint64_t* off_r, uint32_t n_q, const uint32_t* f_idx, const uint32_t* r_idx, uint32_t* r_only,
                                        uint64_t* counts, uint64_t* off_m);
hipError_t msc_launch_pair_strand_write(hipStream_t st, const uint64_t* off_f, const uint64_t* off_r, const uint64_t* off_m, uint32_t n_q, const uint32_t* f_idx, const double* f_sim,
                                        const uint32_t* r_idx, const double* r_sim, const uint32_t* r_only, uint32_t* out_idx, double* out_sim, uint8_t* out_strand);
// the cut of msc_search_pairs_top: each query's place in the list (it keeps min(pairs, top_n); *base grows by their sum), then -- once the
// list has that room -- the selection out of the block's staged pairs (seg[chunk][query] = {first, n}) straight to those places
hipError_t msc_launch_pair_top_plan(hipStream_t st, const uint64_t* seg, uint32_t n_chunks, uint32_t n_q, uint32_t top_n, uint64_t* base, uint64_t* dst);
hipError_t msc_launch_pair_top_select(hipStream_t st, const uint64_t* seg, uint32_t n_chunks, uint32_t n_q, uint32_t top_n, const uint64_t* dst, const uint32_t* s_idx,
                                      const double* s_sim, uint32_t* out_idx, double* out_sim);
// the window bookkeeping the fused epilogue + reduce kernels do for msc_get_close_window (msc_window.hip): pos[i] = position of candidate i,
// alive[] = the window's flags, counter / out = the host-visible list of closed positions (out[0] = best position + 1, out[2 ..] = the list)
struct MscCloseList {
	const uint32_t* pos;
	uint8_t* alive;
	uint32_t* counter;
	uint32_t* out;
	uint32_t* out_host = nullptr;      // the host's own pointer to `out` (page-locked memory the device addresses)
};
// what a workgroup of the fused epilogue + reduce kernel leaves of its candidates: its best (index and, in a window pass, position + 1), its count of
// close ones, its first error. Folded by k_pair_reduce_fold2 -- or, host_parts != nullptr (page-locked, device-addressable), by the caller
// once it has waited for the stream: a launch less per pass of the step-serial loop.
struct ReducePart { double sim; int64_t pos; unsigned long long nclose; int err; uint32_t wpos; };
hipError_t msc_launch_epilogue_reduce(hipStream_t st, const MscEpilogueArgs& a, int mode, int64_t begin, uint8_t* flags_out, MscReduceOut* out, void* parts_scratch,
                                      const MscCloseList& cl, ReducePart* host_parts = nullptr, uint32_t* n_parts_out = nullptr);
// ... the fold of those parts on the host (the arithmetic of k_pair_reduce_fold2); *wpos_out = the best candidate's window position + 1 (0: none)
void msc_reduce_fold_host(const ReducePart* parts, uint32_t n_parts, int mode, MscReduceOut* out, uint32_t* wpos_out);
hipError_t msc_launch_reduce(hipStream_t st, const MscPairOut* pair_out, uint32_t m, int mode, int64_t begin,
                             uint8_t* flags_out, MscReduceOut* out, void* parts_scratch = nullptr, const uint32_t* key = nullptr);
size_t msc_reduce_scratch_bytes();

hipError_t msc_launch_sparse_count(hipStream_t st, const void* scratch_bins, const MscLayout& L, int dtype, uint32_t n, uint64_t* counts);
hipError_t msc_launch_sparse_write(hipStream_t st, const void* scratch_bins, const MscLayout& L, int dtype, uint32_t n, const MscSparseHdr* hdr,
                                   uint64_t first_slot, const uint64_t* cum_base, void* ent, uint32_t* cum);
hipError_t msc_launch_pair_sparse(hipStream_t st, const void* c_ent, const uint32_t* c_cum, const MscSparseHdr* c_hdr, const uint8_t* cand_scalars,
                                  uint64_t scalar_stride, const uint32_t* cand_slots, uint32_t m, const void* q_ent, const uint32_t* q_cum,
                                  const MscSparseHdr* q_hdr, const uint8_t* q_scalars, uint64_t nbins, int use_window, uint64_t min_len,
                                  uint64_t max_len, MscPartial* partials, void* div_tables, void* div_partials, int order);
hipError_t msc_launch_pair_sparse_lds(hipStream_t st, const void* c_ent, const uint32_t* c_cum, const MscSparseHdr* c_hdr, const uint8_t* cand_scalars,
                                      uint64_t scalar_stride, const uint32_t* cand_slots, uint32_t m, const void* q_ent, const uint32_t* q_cum,
                                      const MscSparseHdr* q_hdr, const uint8_t* q_scalars, uint64_t nbins, uint32_t q_nnz, uint32_t max_c_nnz, int use_window,
                                      uint64_t min_len, uint64_t max_len, MscPartial* partials, void* div_tables, void* div_partials, int order, int num_cus);
uint32_t msc_sparse_mp_max_entries();
bool msc_sparse_wl_fits(uint32_t q_nnz, uint32_t c_max_nnz);      // the whole-list kernel takes this 1 x M pass (one record per candidate)
uint32_t msc_sparse_mp_parts(uint32_t m, uint64_t entries, int num_cus, bool div = false);      // waves per candidate for a window of m (1 .. 16)
uint32_t msc_sparse_mp_div_records(uint64_t entries);      // {jd, js} records per pair the merge-path kernel's divergence form writes
hipError_t msc_launch_pair_sparse_mp(hipStream_t st, const void* c_ent, const uint32_t* c_cum, const MscSparseHdr* c_hdr, const uint8_t* cand_scalars,
                                     uint64_t scalar_stride, const uint32_t* cand_slots, uint32_t m, const void* q_ent, const uint32_t* q_cum,
                                     const MscSparseHdr* q_hdr, const uint8_t* q_scalars, uint64_t nbins, int use_window, uint64_t min_len,
                                     uint64_t max_len, MscPartial* partials, void* div_tables, void* div_partials, int order, int num_cus, uint32_t max_total, uint32_t parts, uint32_t q_nnz = 0, uint32_t c_max_nnz = 0,
                                     uint32_t div_stride = 1);
hipError_t msc_launch_sparse_build_sort(hipStream_t st, int k, int dtype, uint64_t nbins, uint64_t first_slot, uint32_t n_seqs, const uint32_t* packed,
                                        const uint64_t* seg_start, const uint64_t* kmer_off, const uint64_t* seq_seg_begin, const uint64_t* seq_arena_off,
                                        uint32_t P, uint8_t* scalars, uint64_t scalar_stride, MscSparseHdr* hdr, void* ent, uint32_t* cum);
hipError_t msc_launch_sparse_scatter(hipStream_t st, const void* ent, const MscSparseHdr* hdr, const uint32_t* slots, uint32_t m, uint32_t* acc);
hipError_t msc_launch_pair_sparse_mp_pairs(hipStream_t st, const void* c_ent, const uint32_t* c_cum, const MscSparseHdr* c_hdr, const uint8_t* cand_scalars,
                                           uint64_t scalar_stride, const uint32_t* cand_slots, uint32_t m, const void* q_ent, const uint32_t* q_cum,
                                           const MscSparseHdr* q_hdr, uint64_t nbins, int use_window, const MscBatchSeg* segs, const uint32_t* pair_seg,
                                           MscPartial* partials, int order, int num_cus, const uint8_t* q_scalars = nullptr, uint64_t q_scalar_stride = 0,
                                           void* div_tables = nullptr, void* div_partials = nullptr, uint32_t div_stride = 1);
// the whole-list kernel for a pair list (k_pair_sparse_wl_pairs): the fit rule over the two sets' longest lists, the largest sum of the
// two it admits, and the launch (integer records only, no window; c_max_nnz / q_max_nnz size a wave's LDS region)
bool msc_sparse_wl_pairs_fits(uint32_t a_max_nnz, uint32_t b_max_nnz);
uint32_t msc_sparse_wl_pairs_limit();
hipError_t msc_launch_pair_sparse_wl_pairs(hipStream_t st, const void* c_ent, const uint32_t* c_cum, const MscSparseHdr* c_hdr, const uint32_t* cand_slots, uint32_t m,
                                           const void* q_ent, const uint32_t* q_cum, const MscSparseHdr* q_hdr, const MscBatchSeg* segs, const uint32_t* pair_seg,
                                           uint32_t c_max_nnz, uint32_t q_max_nnz, uint64_t nbins, MscPartial* partials, int num_cus);
hipError_t msc_launch_sparse_scatter_batch(hipStream_t st, const void* ent, const MscSparseHdr* hdr, const uint32_t* slots, const uint32_t* seg, uint32_t n_members,
                                           uint64_t nbins, uint32_t* acc, uint32_t* touched = nullptr);
// (m_of == nullptr: one centre of m_one members; touched == nullptr: the sweeps over all bins)
hipError_t msc_launch_sparse_mean_count_batch(hipStream_t st, const uint32_t* acc, uint64_t nbins, uint32_t n_chunks, uint64_t chunk_bins, uint32_t n_centres,
                                              const uint32_t* m_of, uint32_t m_one, uint64_t* counts, const uint32_t* touched);
hipError_t msc_launch_sparse_mean_write_batch(hipStream_t st, uint32_t* acc, uint64_t nbins, uint32_t n_chunks, uint64_t chunk_bins, uint32_t n_centres,
                                              const uint32_t* m_of, uint32_t m_one, const uint64_t* chunk_off, const uint64_t* chunk_cum, void* ent, uint32_t* cum,
                                              uint32_t* touched);
hipError_t msc_launch_sparse_assign_batch(hipStream_t st, void* d_ent, uint32_t* d_cum, MscSparseHdr* d_hdr, const void* s_ent, const uint32_t* s_cum, const MscSparseHdr* s_hdr,
                                          const uint32_t* ds, const uint32_t* ss, const uint64_t* dst_off, uint32_t n);
hipError_t msc_launch_assign_scalars(hipStream_t st, uint8_t* dst_scalars, const uint8_t* src_scalars, uint64_t stride_bytes, const uint32_t* dst_slots,
                                     const uint32_t* src_slots, uint32_t n, int exact = 0);
hipError_t msc_launch_pair_sparse_groups(hipStream_t st, const void* c_ent, const MscSparseHdr* c_hdr, const uint8_t* cand_scalars, uint64_t scalar_stride,
                                         const uint32_t* cand_slots, uint32_t m, const void* q_ent, const MscSparseHdr* q_hdr, int use_window, uint64_t min_len,
                                         uint64_t max_len, double* out);
hipError_t msc_launch_sparse_nnz_sum(hipStream_t st, const MscSparseHdr* hdr, const uint8_t* cand_scalars, uint64_t scalar_stride, const uint32_t* slots, uint64_t first_slot,
                                     uint32_t m, int use_window, uint64_t min_len, uint64_t max_len, uint64_t* acc);
hipError_t msc_launch_sparse_self_markov(hipStream_t st, const void* ent, const MscSparseHdr* hdr, const uint32_t* slots, uint64_t first_slot, uint32_t m, double* out);
// the same records from tile-permuted dense slots, for histograms under 64 KiB (pair_features.hip)
hipError_t msc_launch_pair_groups_dense(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* c_bins, const uint8_t* cand_scalars, uint64_t scalar_stride,
                                        const uint32_t* cand_slots, uint32_t m, const uint8_t* q_bins, int use_window, uint64_t min_len, uint64_t max_len, double* out);
hipError_t msc_launch_self_markov_dense(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* bins, const uint32_t* slots, uint64_t first_slot, uint32_t m,
                                        double* out);
hipError_t msc_launch_colsum(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* bins,
                             const uint32_t* member_slots, uint32_t m, void* rounded_out /*T, physical*/,
                             double* mean_out /*physical, nullable*/, uint64_t* floor_sum_out, uint64_t* scratch);
hipError_t msc_launch_distance_d(hipStream_t st, const MscPartial* partials, uint32_t S, uint32_t m,
                                 const uint8_t* scalars, uint64_t scalar_stride, const uint32_t* member_slots,
                                 const uint8_t* r_scalars, const uint64_t* floor_sum, double* dist_out,
                                 MscReduceOut* out);
// batched forms for msc_update_centres: one (query, candidate list) problem per segment
hipError_t msc_launch_pair_tiles_batch(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* cand_bins, const uint8_t* cand_scalars,
                                       const uint32_t* cand_slots, const MscBatchSeg* segs, uint32_t n_segs, uint32_t max_m, const uint8_t* qset_bins,
                                       uint64_t q_slot_bytes, const uint8_t* qset_scalars, uint64_t q_scalar_stride, int use_window, MscPartial* partials,
                                       int order);
hipError_t msc_launch_colsum_batch(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* bins, const uint32_t* member_slots, const MscBatchSeg* segs,
                                   uint32_t n_segs, void* rounded_out, uint64_t* floor_sum_out);
hipError_t msc_launch_colsum_sums(hipStream_t st, const MscLayout& L, int dtype, const uint8_t* bins, const uint32_t* member_slots, const MscBatchSeg* segs, uint32_t n_segs,
                                  uint64_t* sums_out);
hipError_t msc_launch_mean_from_sums(hipStream_t st, const MscLayout& L, int dtype, const uint64_t* sums, const uint64_t* m_total, uint32_t n_segs, void* rounded_out,
                                     uint64_t* floor_sum_out);
hipError_t msc_launch_distance_batch(hipStream_t st, const MscPartial* partials, uint32_t S, uint32_t n, const uint8_t* scalars, uint64_t scalar_stride,
                                     const uint32_t* member_slots, const uint32_t* pair_seg, const uint8_t* r_scalars, uint64_t r_stride, const uint64_t* floor_sum,
                                     double* dist_out);
hipError_t msc_launch_assign_batch(hipStream_t st, const MscLayout& L, uint8_t* dst_bins, uint8_t* dst_scalars, const uint8_t* src_bins,
                                   const uint8_t* src_scalars, const uint32_t* dst_slots, const uint32_t* src_slots, uint32_t n, int exact = 0);
// msc_revcomp.hip: the reverse complement of slots, bins'[b] = bins[msc_rc_bin(b)]. Dense: the bins (whole in LDS up to 64 KiB a slot, else as a
// tiled transpose), the tile prefixes of the new bins and the reversed 1-mers; the rest of the record is the caller's (msc_launch_assign_scalars)
bool msc_revcomp_whole_slot(const MscLayout& L);
hipError_t msc_launch_hist_revcomp(hipStream_t st, const MscLayout& L, int k, int dtype, uint8_t* dst_bins, uint8_t* dst_scalars, const uint8_t* src_bins,
                                   const uint8_t* src_scalars, const uint32_t* dst_slots, const uint32_t* src_slots, uint32_t n);
hipError_t msc_launch_revcomp_one_mers(hipStream_t st, uint8_t* dst_scalars, const uint8_t* src_scalars, uint64_t stride, const uint32_t* dst_slots,
                                       const uint32_t* src_slots, uint32_t n);
// sparse: lists of at most msc_sparse_revcomp_sort_max() entries sorted in LDS (list i of the launch goes to dst_off[i] of the arena); a longer
// one scattered into a dense slot that holds the pseudocount, for k_sparse_count / k_sparse_write
uint32_t msc_sparse_revcomp_sort_max();
hipError_t msc_launch_sparse_revcomp_sort(hipStream_t st, int k, uint64_t nbins, const void* s_ent, const MscSparseHdr* s_hdr, const uint32_t* dst_slots,
                                          const uint32_t* src_slots, const uint64_t* dst_off, uint32_t n, uint32_t longest, void* d_ent, uint32_t* d_cum, MscSparseHdr* d_hdr,
                                          MscSparseHdr* hdr_list);
hipError_t msc_launch_sparse_revcomp_scatter(hipStream_t st, const MscLayout& L, int k, int dtype, void* scratch_bins, const void* ent, uint32_t n);
// msc_canonical.hip: canon(D)[b] = clamp(D[b] + D[msc_rc_bin(b)] - 1, 0, max(T)) for slots, in place where a pair names one slot twice. Dense: the
// record's words that do not follow from the bins (msc_launch_canonical_record: length, id, overflow, n_kmers, the 1-mers added up), then the bins,
// which set the record's overflow word where a sum saturates; the sums and tile prefixes are msc_launch_finalize's, called by the API afterwards
hipError_t msc_launch_canonical_record(hipStream_t st, uint8_t* dst_scalars, const uint8_t* src_scalars, uint64_t stride, const uint32_t* dst_slots, const uint32_t* src_slots,
                                       uint32_t n);
hipError_t msc_launch_hist_canonical(hipStream_t st, const MscLayout& L, int k, int dtype, uint8_t* dst_bins, uint8_t* dst_scalars, const uint8_t* src_bins,
                                     const uint8_t* src_scalars, const uint32_t* dst_slots, const uint32_t* src_slots, uint32_t n);
// sparse: counts[i] = the entries of the merged list of src_slots[i]; lists of at most msc_sparse_canonical_sort_max() entries merged and sorted in
// LDS (list i of the launch goes to dst_off[i] of the arena; the record's sums are written too, after msc_launch_canonical_record)
uint32_t msc_sparse_canonical_sort_max();
hipError_t msc_launch_sparse_canonical_count(hipStream_t st, int k, const void* s_ent, const MscSparseHdr* s_hdr, const uint32_t* src_slots, uint32_t n, uint32_t* counts);
hipError_t msc_launch_sparse_canonical_sort(hipStream_t st, int k, int dtype, uint64_t nbins, const void* s_ent, const MscSparseHdr* s_hdr, const uint32_t* dst_slots,
                                            const uint32_t* src_slots, const uint64_t* dst_off, uint32_t n, uint32_t longest, void* d_ent, uint32_t* d_cum, MscSparseHdr* d_hdr,
                                            MscSparseHdr* hdr_list, uint8_t* dst_scalars, uint64_t scalar_stride);
