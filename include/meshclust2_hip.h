/* include/meshclust2_hip.h
 *
 * C ABI of libmeshclust2_hip.so: the MI355X (gfx950) replacement for MeShClust2's alignment-free
 * pairwise-identity hot path. Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * The reference (BioinformaticsToolsmith/MeShClust2 v2.3.0) has no FFI layer: the path is reached through
 * C++ template member calls. Each entry point below names the reference call site(s) it replaces
 * (file:line relative to the reference's src/). INTEGRATION.md shows the shim a maintainer would add on
 * the reference side.
 *
 * Conventions
 *   - every function returns MSC_OK (0) or a negative msc_status; msc_last_error(ctx) has the message.
 *     Nothing throws across the ABI (the reference throws std::exception / const char* / int).
 *   - a msc_ctx owns one HIP device + one stream and is NOT thread-safe: use one ctx per host thread
 *     (the reference calls compute()/classify() from OpenMP workers on shared read-only state,
 *     cluster/Trainer.cpp:41,84).
 *   - calls are synchronous: results are valid when the call returns.
 *   - histograms live in HBM inside a msc_hist_set from the moment they are built; the host sees
 *     slot indices, flags and scalars. `dtype` is the reference's --datatype: 8, 16, 32 or 64
 *     (cluster/CRunner.cpp:108-126), fixed per set.
 *   - there is NO CPU fallback: msc_create() fails with MSC_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef MESHCLUST2_HIP_H
#define MESHCLUST2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSC_ABI_VERSION 1

typedef enum {
	MSC_OK = 0,
	MSC_ERR_INVALID_ARG = -1,
	MSC_ERR_NO_DEVICE = -2,       /* no usable gfx950 device / HIP runtime error at init */
	MSC_ERR_HIP = -3,             /* a HIP call failed; message has hipGetErrorString */
	MSC_ERR_OOM = -4,
	MSC_ERR_INVALID_INPUT = -5,   /* InvalidInputException: character outside the IUPAC map (nonltr/ChromosomeOneDigit.cpp:86-94) */
	MSC_ERR_ZERO_LENGTH = -6,     /* `throw 123`: length_difference on a zero-length point (predict/Feature.cpp:878-886) */
	MSC_ERR_NAN = -7,             /* normalize_cache found NaN (predict/Feature.cpp:143-146) */
	MSC_ERR_UNSUPPORTED = -8,     /* feature flag outside the 11 in-scope statistics, k out of range, ... */
	MSC_ERR_IO = -9
} msc_status;

/* Single-feature bits: identical values to FEAT_* in predict/Feature.h:31-64. */
#define MSC_FEAT_MANHATTAN          (1ULL << 2)
#define MSC_FEAT_EUCLIDEAN          (1ULL << 3)
#define MSC_FEAT_NORMALIZED_VECTORS (1ULL << 5)
#define MSC_FEAT_JEFFEREY_DIV       (1ULL << 7)
#define MSC_FEAT_PEARSON_COEFF      (1ULL << 9)
#define MSC_FEAT_INTERSECTION       (1ULL << 13)
#define MSC_FEAT_EMD                (1ULL << 18)
#define MSC_FEAT_LENGTHD            (1ULL << 21)
#define MSC_FEAT_KULCZYNSKI2        (1ULL << 27)
#define MSC_FEAT_SIMRATIO           (1ULL << 28)
#define MSC_FEAT_JENSEN_SHANNON     (1ULL << 29)
/* PRED_FEAT_FAST / PRED_FEAT_DIV, predict/Predictor.h:23-24 (`--feat fast` = FAST, `--feat slow` = FAST|DIV) */
#define MSC_FEAT_FAST (MSC_FEAT_EUCLIDEAN | MSC_FEAT_MANHATTAN | MSC_FEAT_INTERSECTION | MSC_FEAT_KULCZYNSKI2 | \
                       MSC_FEAT_SIMRATIO | MSC_FEAT_NORMALIZED_VECTORS | MSC_FEAT_PEARSON_COEFF | MSC_FEAT_EMD | MSC_FEAT_LENGTHD)
#define MSC_FEAT_DIV  (MSC_FEAT_JEFFEREY_DIV | MSC_FEAT_JENSEN_SHANNON)
#define MSC_FEAT_SLOW (MSC_FEAT_FAST | MSC_FEAT_DIV)
/* Two of the reference's `extraslow` statistics (PRED_FEAT_ALL, predict/Predictor.h:25): sums over the groups of four neighbouring
 * bins that share a (k-1)-mer prefix. rre_k_r: predict/Feature.cpp:1029-1062; sim_mm = 1 - exp((d_markov(a,b) + d_markov(b,a)) / 2)
 * with Feature<T>::markov, :1367-1393,1429-1455. Scored on sorted (bin, value) lists (sparse sets, and dense sets of histograms
 * >= 64 KiB through their sparse mirror) or, for smaller histograms, straight from the dense slots -- same terms, same order;
 * usable in msc_pair_features_raw, msc_score, the Trainer operators and models, not in msc_train_class. */
#define MSC_FEAT_RRE_K_R            (1ULL << 14)
#define MSC_FEAT_SIM_MM             (1ULL << 16)
#define MSC_FEAT_GROUPS (MSC_FEAT_RRE_K_R | MSC_FEAT_SIM_MM)

/* Combo codes as written in the weights file (predict/Predictor.cpp:96-110). */
#define MSC_COMBO_XY   0
#define MSC_COMBO_XY2  1
#define MSC_COMBO_X2Y  2
#define MSC_COMBO_X2Y2 3

#define MSC_MAX_SINGLES 16
#define MSC_MAX_COMBOS  8

/* Argument order of a scored pair. All 11 statistics are symmetric EXCEPT the reference's uint32_t
 * simratio (its wrapped difference), so the order is part of the contract:
 *   MSC_ORDER_CAND_FIRST : f(candidate, query)  -- Trainer::get_close, merge (cluster/Trainer.cpp:49,93)
 *   MSC_ORDER_QUERY_FIRST: f(query, candidate)  -- Trainer::filter -> classify(p, pt) (cluster/Trainer.cpp:133) */
#define MSC_ORDER_CAND_FIRST  0
#define MSC_ORDER_QUERY_FIRST 1

typedef struct msc_ctx msc_ctx;
typedef struct msc_hist_set msc_hist_set;
typedef struct msc_model msc_model;

/* Scalar members of one DivergencePoint<T> (clutil/DivergencePoint.h:81-87) plus derived sums the kernels use. */
typedef struct {
	uint64_t mag;          /* DivergencePoint::mag as the reference holds it (stale after hist_assign) */
	uint64_t length;       /* effective length (Chromosome::getEffectiveSize) */
	uint64_t sum;          /* true sum of the bins */
	uint64_t sum_sq;       /* sum of squared bins */
	uint64_t max_count;    /* largest bin */
	uint64_t one_mers[4];  /* k=1 table with pseudocount 1 (clutil/Loader.cpp:143-153) */
	double   stddev;       /* clutil/Loader.cpp:158-171 */
	int32_t  overflow;     /* 1 if some bin saturated at max(T) (nonltr/KmerHashTable.cpp:248-252) */
	int32_t  pad_;
	uint64_t id;
} msc_hist_info;

/* ------------------------------------------------------------------ context */
int         msc_abi_version(void);
/* device >= 0: HIP ordinal. Fails (MSC_ERR_NO_DEVICE) if HIP cannot initialise that device. */
int         msc_create(int device, msc_ctx** out);
void        msc_destroy(msc_ctx* ctx);
const char* msc_last_error(const msc_ctx* ctx);     /* ctx may be NULL: last error of a failed msc_create */
int         msc_device_name(const msc_ctx* ctx, char* buf, size_t cap);
int         msc_synchronize(msc_ctx* ctx);
/* Wall-clock of the dominant kernel (pair_tiles) of the LAST scoring call, from HIP events on the ctx stream (ms). */
int         msc_last_kernel_ms(const msc_ctx* ctx, float* pair_tiles_ms, float* total_ms);
/* The events behind msc_last_kernel_ms cost four records per 1 x M call: a step-serial caller (the accumulate loop issues one
 * Trainer::get_close per step) switches them off; msc_last_kernel_ms then fails with MSC_ERR_INVALID_ARG. Default: on. */
int         msc_set_kernel_timing(msc_ctx* ctx, int on);
/* A dense set whose histograms have a list form (64 KiB and more) keeps a sparse mirror of its slots, and its 1 x M passes
 * (Trainer::get_close / filter / merge, Feature::compute: cluster/Trainer.cpp:23-141) merge the two lists -- 8 bytes per counted k-mer
 * instead of 4^k bins per candidate, same integer reductions. on = 0 keeps those passes on the streaming kernel over the bins (the
 * 1 x M shape SURVEY 8(d) prices at 4^k sizeof(T) bytes per pair); results are identical either way. Default: on
 * (off at start with MSC_NO_MIRROR_1XM in the environment). */
int         msc_set_mirror_pass(msc_ctx* ctx, int on);
/* msc_score_multi queues the blocks of a call (128 queries x all candidates each; fastcar's outer loop, fastcar/FC_Runner.cpp:585-597) on
 * three streams: block i's product beside its rank walk, the epilogue of block i - 1 and the queries' side of block i + 1. on = 0 runs
 * every kernel of a block on ONE stream, block after block: same results, and per-kernel timings (msc_last_kernel_ms, rocprofv3) that are
 * not stretched by a neighbour -- what the roofline of the product kernel is measured on. Default: on (off at start with
 * MSC_GEMM_NO_PIPE in the environment). */
int         msc_set_block_pipe(msc_ctx* ctx, int on);
/* msc_search_pairs sends a model that holds jefferey_divergence or jensen_shannon (every --feat slow model) through msc_score_multi block by
 * block, whose divergence sums come from the sparse merge kernels. on = 1 keeps such a call on the matrix-core route instead (where that
 * route's other conditions hold; a model with sim_mm or rre_k_r still takes the fallback): the two sums are evaluated per pair from exact
 * (count, count) cell counts and the lists of large bins, in one fixed order, so a pair's value does not depend on blocks, chunks, the slot
 * list or the windows. That order is not the merge kernels': the similarities agree with the fallback's to rounding (1e-9 relative), NOT bit
 * for bit, and a pair whose weighted sum sits within rounding of the threshold may be listed by one route only. msc_pairs_info.route reports
 * MSC_PAIRS_ROUTE_MATRIX, and msc_last_kernel_info's name says that the sums came from cells. msc_score_multi and every other call are
 * unaffected (msc_score_multi has a switch of its own, msc_set_multi_div_cells; the two are independent). Default: off. */
int         msc_set_pairs_div_cells(msc_ctx* ctx, int on);
/* msc_score_multi queues one merge pass per query behind the matrix product when the model's singles or feat_mask hold
 * jefferey_divergence or jensen_shannon (every --feat slow model): the two sums come from the sparse merge kernels over the sets' sparse
 * mirrors. on = 1 keeps a block of such a call on the matrix-core route with NO pass between the product and the epilogue: the epilogue
 * evaluates the two sums per pair from exact (count, count) cell counts and the lists of large bins, as msc_search_pairs does under
 * msc_set_pairs_div_cells, and fills every output -- sums, classify sums, flags, close counts (msc_last_close_counts answers), raw
 * statistics with the two divergence columns beside the others. The route's other conditions are unchanged (8/16/32-bit sets of the
 * narrow range in whole 4 KiB tiles, n_q >= 2, a hot list within its bound, ranks mirrors when emd is wanted); it then also serves
 * histograms under 64 KiB, which have no list form (k = 7 with 16-bit bins), two sparse sets under msc_set_sparse_matrix_pass, and the
 * three-stream block pipe; a dense set whose blocks all take it builds no sparse mirror. What goes on exactly as with the switch off --
 * same kernels, names and bits: a model or feat_mask with sim_mm or rre_k_r, a block whose hot list is too long, a set off the matrix
 * route (k = 5, wide counts, k = 13, padded tiles), a single query, mirrors that cannot be allocated.
 * Values: every statistic other than the two divergence sums is bit-equal to the switch-off call's (the same exact integers). The two
 * sums, and what a model derives from them, agree with the switch-off call and with the reference to 1e-9 relative (1e-13 absolute), NOT
 * bit for bit: the order of the FP64 additions is not the merge kernels'. A pair whose weighted sum lies within that rounding of zero may
 * get the other flag. A pair's value depends on the pair alone -- not on its block, the chunk of candidates, the slot list, the block pipe
 * or dense versus sparse sets -- and has the bits msc_search_pairs with msc_set_pairs_div_cells gives that pair. Error statuses and NaN
 * rows (zero length, NaN) are the switch-off call's. msc_last_kernel_info names the product kernel and adds "divergence sums from
 * cells". msc_search_pairs's own matrix route follows msc_set_pairs_div_cells alone; its fallback IS a sequence of msc_score_multi calls
 * and follows this switch as they do. No other call is affected. Default: off. */
int         msc_set_multi_div_cells(msc_ctx* ctx, int on);
/* A msc_score_multi call that wants nothing but the close flags, on the matrix-core route with a model that holds
 * earth_movers_distance: the flags are first decided from exact integer bounds of that distance (two moments per slot of the ranks
 * mirror), and the rank lists are walked only for the pairs the bounds leave open -- a device list of at most 1/64 of a block's pairs,
 * evaluated in FP64 with their exact distances. A block whose list overflows is scored as with the switch off, on the device, without a
 * host round trip; a model more than half of whose blocks overflowed in one call is remembered, and later calls with it skip the bound
 * pass. The flags are those of the switch-off call, pair for pair. on = 0: the distance of every pair of a block is formed first (the
 * path before this switch existed). Default: on (off at start with MSC_NO_EMD_BOUNDS in the environment). Calls that want sums,
 * classify sums or raw statistics, --feat slow models, msc_search_pairs* and msc_score_pair_list do not look at it. */
int         msc_set_emd_bounds(msc_ctx* ctx, int on);
/* What the last msc_score_multi call did about the earth mover's distance of its close-flag blocks (those the switch above is about):
 * blocks = such blocks, dense_blocks = those whose every pair had its rank lists walked (switch off, a remembered model, sets of
 * different list pitch, an overflowed list), listed_pairs = pairs walked one by one from the lists of the others. A block whose candidates
 * run in several chunks (one launch's scratch is capped) counts once PER CHUNK in blocks and dense_blocks: each chunk has a list of its own,
 * 1/64 of the chunk's pairs, and overflows or not by itself; the rule that remembers a model counts chunks on both sides. Any pointer may be null. */
int         msc_last_emd_walk(const msc_ctx* ctx, uint64_t* listed_pairs, uint64_t* dense_blocks, uint64_t* blocks);
/* The blocks the switch above is about multiply presence bits of every pair of a block on the matrix cores to count its shared k-mers, which
 * all but the related pairs' flags do not need exactly. fold = 8, 16 or 32 (default 16; 0 at start with MSC_NO_FOLD in the environment): the
 * product of such a block runs over bits folded fold-to-1 -- an upper bound of the shared k-mers at 1/fold of the work --, the screen decides
 * from intervals, and the pairs it leaves open get their exact counts one by one. A block whose list of open pairs overflows is scored
 * again by the true product once the call's blocks are through; a model most of whose blocks do so is remembered. Sets whose histograms are too small to fold (k = 5) and
 * every other call keep their route. The flags are those of fold = 0, pair for pair. Any other value of fold: MSC_ERR_INVALID_ARG. */
int         msc_set_fold_screen(msc_ctx* ctx, int fold);
/* The queries' side of the matrix-core blocks of msc_score_multi (their bits as the product's tiles and transposed, their lists of large bins by step) is
 * built for up to `cap` consecutive full blocks in one set of launches, a group ahead of the blocks that read it (default 32; 0 at start with
 * MSC_NO_QUERY_GROUPS in the environment). cap = 0 or 1: block by block. Identical results. cap < 0: MSC_ERR_INVALID_ARG. */
int         msc_set_query_groups(msc_ctx* ctx, int cap);
/* The folded blocks of msc_score_multi (msc_set_fold_screen) run what follows their product -- the screen, the listed pairs' exact counts, walk and FP64
 * evaluation, the close counts, the flags' copy home -- once for up to `cap` consecutive full blocks of one query group (default 8; 0 at start with
 * MSC_NO_TAIL_GROUPS in the environment). The call's final groups halve down to one block (MSC_TAIL_NO_RAMP in the environment: full groups to the end).
 * cap = 0 or 1: block by block. Identical results and counters. cap < 0: MSC_ERR_INVALID_ARG. */
int         msc_set_tail_groups(msc_ctx* ctx, int cap);
/* What the last msc_score_multi call did about it: the tail groups of two blocks and more it ran, and the blocks in them. Any pointer may be null. */
int         msc_last_tail_groups(const msc_ctx* ctx, uint64_t* groups, uint64_t* grouped_blocks);
/* What the last msc_score_multi call did about it: the fold used (0: none), the blocks whose product was folded, and those of them that fell
 * back to the true product. Any pointer may be null. */
int         msc_last_fold_screen(const msc_ctx* ctx, uint64_t* fold, uint64_t* folded_blocks, uint64_t* fell_back);
/* A folded block decides most of its pairs without an evaluation: per query row an integer cut T(q) is PROVEN once per block (csrc/msc_fold_reject.h: for
 * every candidate within the ranges of the candidates' set whose folded product output P1' + P2' is at most T(q), an upper bound of the model's sum
 * lies below 0), and the screen evaluates only the waves that hold a pair above the cut or a row without one. on = 1 (default; 0 at start with
 * MSC_NO_FOLD_REJECT in the environment). The flags are those of on = 0, pair for pair. */
int         msc_set_fold_reject(msc_ctx* ctx, int on);
/* What the last msc_score_multi call did about it: the pairs of its folded blocks the cut rejected, and the query rows of those blocks that got no cut.
 * Any pointer may be null. */
int         msc_last_fold_reject(const msc_ctx* ctx, uint64_t* rejected_pairs, uint64_t* rows_without_cut);
/* The fold map: the folded bin of `bin` of a histogram of nbins = 4^k bins, bin mod (nbins / fold); fold a power of two (0, 1: bin). */
uint64_t    msc_fold_bin(uint64_t bin, uint64_t nbins, uint32_t fold);
/* A Q x M call over two SPARSE sets (msc_score_multi, msc_search_pairs) runs one 1 x M pass per query over the lists: the matrix-core
 * route reads a presence bit per bin, the lists of large bins and the sorted ranks of a set -- mirrors only dense sets used to carry.
 * on = 1 lets two sparse sets of equal k and dtype take that route as well, under its usual conditions (8/16/32-bit bins of the narrow
 * range, whole 4 KiB tiles, two queries and more) and up to k = 10: the three mirrors are built from the lists, byte for byte what a dense
 * set of the same sequences builds from its bins, so the products, rank walks and epilogues run unchanged and every result -- statistics,
 * sums, flags, close counts, the pair list -- equals both the switch-off call's and the dense sets'. The mirrors are allocated by the
 * first call that takes the route (a bit per bin and slot, 8 bytes per large bin, 4 + 2 bytes per rank) and every writer of a slot's list
 * makes that slot stale in them. A block whose queries' list of large bins is too long, a set whose mirrors cannot be allocated, and in
 * msc_score_multi a model or feat_mask with a divergence or group statistic go on as without the switch, with the same kernels (in
 * msc_search_pairs a divergence-statistic model takes the route where msc_set_pairs_div_cells is on as well). msc_last_kernel_info names
 * the product kernel and adds "mirrors from lists". One dense and one sparse set are not affected. Default: off. */
int         msc_set_sparse_matrix_pass(msc_ctx* ctx, int on);
/* Number of streaming-kernel launches that pair_tiles_ms sums over (large calls are chunked). */
int         msc_last_kernel_launches(const msc_ctx* ctx);
/* Which streaming kernel the LAST scoring call ran (its name is copied to buf) and how many queries one HBM read of a
 * candidate tile served in it (1 for the 1 x M passes): the figure the algorithmic bytes of a Q x M launch divide by. */
int         msc_last_kernel_info(const msc_ctx* ctx, char* buf, size_t cap, int* queries_per_candidate_read);

/* ------------------------------------------------------------------ a1: sequence encoding (host byte work)
 * Replaces Chromosome::help / removeAmbiguous / mergeSegments / makeSegmentList + ChromosomeOneDigit::encode
 * (nonltr/Chromosome.cpp:130-154,263-385; nonltr/ChromosomeOneDigit.cpp:79-133).
 * codes_out[len]: 0..3 where the reference encodes, raw 'N' elsewhere. segs_out: inclusive [s,e] pairs. */
int msc_encode(const char* seq, size_t len, uint8_t* codes_out, int64_t* segs_out, size_t max_segs,
               size_t* n_segs, uint64_t* eff_len);

/* ------------------------------------------------------------------ a2-a4: histogram sets */
/* A set holds `capacity` slots of 4^k bins of `dtype` bits in HBM (tile-permuted layout). */
int      msc_hist_set_create(msc_ctx* ctx, int k, int dtype, uint64_t capacity, msc_hist_set** out);
void     msc_hist_set_destroy(msc_hist_set* set);
uint64_t msc_hist_set_capacity(const msc_hist_set* set);
int      msc_hist_set_k(const msc_hist_set* set);
int      msc_hist_set_dtype(const msc_hist_set* set);
uint64_t msc_hist_set_bytes(const msc_hist_set* set);              /* HBM footprint */

/* SPARSE layout: a slot stores only the bins above the pseudocount, as a sorted (bin, value) list.
 * Same semantics and the same results as a dense set for msc_hist_build*, msc_hist_download (expanded on the host),
 * msc_hist_info_get, clone / assign / copy, msc_pair_features_raw, msc_score(_multi), msc_get_close, msc_filter, msc_merge and
 * msc_search; it is what makes k = 11..15 possible (a dense k = 13 histogram is 64-512 MiB) and it reads 12 bytes per
 * stored bin instead of 4^k * dtype/8 per histogram. max_entries = total stored bins the set can hold (sum over slots, <= the
 * total number of k-mers). Needs 4^k * dtype/8 >= 64 KiB. msc_hist_upload and the mean_out of msc_mean_nearest are not available on sparse sets. */
int      msc_hist_set_create_sparse(msc_ctx* ctx, int k, int dtype, uint64_t capacity, uint64_t max_entries, msc_hist_set** out);
int      msc_hist_set_is_sparse(const msc_hist_set* set);
uint64_t msc_hist_set_entries(const msc_hist_set* set, uint64_t slot);     /* stored bins of one slot (a dense set: of its sparse mirror, 0 before it exists) */
/* Empties a sparse set: every slot back to "never written", the whole entry arena free again. The entry arena is append-only
 * (a slot that is assigned again leaves its old list behind), so a store of moving centres is compacted by copying its live slots
 * into a second set (msc_hist_copy_batch) and clearing the first for the next time -- no allocation in the loop. The reference has
 * no counterpart: its centres are heap objects (Center<T>, cluster/Center.h). Dense sets: MSC_ERR_UNSUPPORTED. */
int      msc_hist_set_clear(msc_ctx* ctx, msc_hist_set* set);

/* Replaces Loader<T>::get_point (clutil/Loader.cpp:112-179; callers cluster/CRunner.cpp:526,
 * predict/Predictor.cpp:799,858, fastcar/FC_Runner.cpp:501) for n_seqs sequences at once.
 *   seqs[i]/lens[i] : raw ASCII sequence i (FASTA body, no header, no newlines).
 *   strip_non_acgt  : 1 = the std::string overload (drops every char that is not upper-case ACGT first,
 *                     Loader.cpp:115-121); 0 = the ChromosomeOneDigit overload used by the clustering CLI.
 * Slots first_slot .. first_slot+n_seqs-1 are overwritten. Host encodes + packs to 2 bits/base, the GPU
 * counts. MSC_ERR_INVALID_INPUT if a sequence holds a character outside the IUPAC map. */
int msc_hist_build(msc_ctx* ctx, msc_hist_set* set, uint64_t first_slot, uint64_t n_seqs,
                   const char* const* seqs, const uint64_t* lens, int strip_non_acgt);

/* Same, from already-encoded input (what a caller with its own FASTA reader hands over):
 *   packed        : 2-bit codes, base b at bits [2*(b%4), 2*(b%4)+1] of byte b/4, all sequences concatenated
 *   seg_seq/start/end : n_segs segments; seg_seq[j] = sequence ordinal, [start,end] inclusive GLOBAL base offsets
 *                    (the reference's segment list, nonltr/Chromosome.cpp:355-385); only k-mers fully inside a
 *                    segment are counted (clutil/Loader.cpp:53-54)
 *   eff_len[i], one_mers[4*i..] : per-sequence effective length and k=1 counts (pseudocount included) */
int msc_hist_build_packed(msc_ctx* ctx, msc_hist_set* set, uint64_t first_slot, uint64_t n_seqs,
                          const uint8_t* packed, uint64_t n_bases,
                          const uint32_t* seg_seq, const uint64_t* seg_start, const uint64_t* seg_end, uint64_t n_segs,
                          const uint64_t* eff_len, const uint64_t* one_mers);

/* The same with `packed` in THIS device's memory (every other array on the host, as above): the form a multi-GPU driver uses for
 * sequences that arrived over xGMI -- fastcar's outer loop hands each chunk of queries to every database chunk
 * (fastcar/FC_Runner.cpp:585-597); with the database sharded over GPUs the chunk's bases are all-gathered device to device and
 * each rank builds the block's histograms itself. `packed` is read on the context's own stream: its bytes must be COMPLETE when the
 * call is made (a producer on another stream -- an RCCL all-gather -- is waited for by the caller first). */
int msc_hist_build_packed_dev(msc_ctx* ctx, msc_hist_set* set, uint64_t first_slot, uint64_t n_seqs,
                              const void* packed_dev, uint64_t n_bases,
                              const uint32_t* seg_seq, const uint64_t* seg_start, const uint64_t* seg_end, uint64_t n_segs,
                              const uint64_t* eff_len, const uint64_t* one_mers);

/* Diagnostics of the builders (tests, profiling): which builder the LAST msc_hist_build* call on this set ran, and the set's current
 * bounds. `builder` (nullable) receives one of these fixed names, "" before the first build:
 *   "k_build_lds"                  dense, 4^k <= 16384 bins: the whole histogram counted in LDS
 *   "k_build_sort"                 dense, larger histograms, <= 32768 k-mers per sequence: the k-mer indices sorted in LDS
 *   "k_count"                      dense, everything else: k_fill + k_count + k_finalize + k_prefix
 *   "k_sparse_build_sort"          sparse, <= 32768 k-mers per sequence: the lists straight from the sorted k-mer indices
 *   "k_count+k_sparse_write"       sparse, everything else: dense scratch slots (built by k_count) compacted by k_sparse_count / k_sparse_write
 *   "k_build_sort+k_sparse_write", "k_build_lds+k_sparse_write"
 *                                  the same where the dense rule gives the scratch slots to another builder (short
 *                                  sequences under MSC_NO_SORT_BUILD, the switch that turns k_sparse_build_sort off)
 * A call that is refused before anything is launched leaves the name as it was. max_count / max_sum (nullable): the largest bin and the
 * largest sum of bins over every slot ever written -- what selects the count width and the wide kernels of the scoring calls; never
 * below the true maxima of the set's slots. max_nnz: the longest list ever stored in a sparse set, 0 for a dense set. */
int msc_hist_set_build_info(const msc_hist_set* set, char* builder, size_t cap,
                            uint64_t* max_count, uint64_t* max_sum, uint64_t* max_nnz);

/* Debug / parity: bins in NATURAL k-mer order (first base most significant), 4^k * dtype/8 bytes. */
int msc_hist_download(msc_ctx* ctx, const msc_hist_set* set, uint64_t slot, void* bins_out);
int msc_hist_upload(msc_ctx* ctx, msc_hist_set* set, uint64_t slot, const void* bins, uint64_t length,
                    const uint64_t* one_mers /* 4 or NULL */);       /* DivergencePoint(pts, len) ctor: mag recomputed */
int msc_hist_info_get(msc_ctx* ctx, const msc_hist_set* set, uint64_t slot, msc_hist_info* out);
/* DivergencePoint::get_length() of n consecutive slots at once (the driver's sort by length, cluster/CRunner.cpp:529-560, reads every
 * point's): served from the lengths the library remembers on the host, or one strided copy. */
int msc_hist_lengths(msc_ctx* ctx, const msc_hist_set* set, uint64_t first_slot, uint64_t n, uint64_t* lengths_out);
int msc_hist_set_id(msc_ctx* ctx, msc_hist_set* set, uint64_t slot, uint64_t id);

/* DivergencePoint::clone (clutil/DivergencePoint.h:35-43): full copy, mag re-summed. Used by Center (cluster/Center.h:13-40). */
int msc_hist_clone(msc_ctx* ctx, msc_hist_set* dst, uint64_t dst_slot, const msc_hist_set* src, uint64_t src_slot);
/* DivergencePoint::set (clutil/DivergencePoint.cpp:182-190; caller cluster/ClusterFactory.cpp:328,331):
 * bins, length and id are copied, `mag` is NOT. */
int msc_hist_assign(msc_ctx* ctx, msc_hist_set* dst, uint64_t dst_slot, const msc_hist_set* src, uint64_t src_slot);
/* center->set(*next) for many centres in one launch (the tail of every mean_shift_update of a round, cluster/ClusterFactory.cpp:328,331):
 * msc_hist_assign(dst, dst_slots[i], src, src_slots[i]) for i < n; the destination slots must be distinct. */
int msc_hist_assign_batch(msc_ctx* ctx, msc_hist_set* dst, const uint32_t* dst_slots, const msc_hist_set* src, const uint32_t* src_slots, uint64_t n);

/* Exact slot copy: bins and EVERY scalar (incl. a stale mag). What a host container of Center objects needs when it
 * relocates them without going through clone() (std::vector growth of the device-side centre store). */
int msc_hist_copy(msc_ctx* ctx, msc_hist_set* dst, uint64_t dst_slot, const msc_hist_set* src, uint64_t src_slot);
/* The same for n slots in one launch per region (relocating or compacting a whole centre store: the vector<Center*> of
 * cluster/ClusterFactory.cpp:560-575 as it grows); the destination slots must be distinct. A sparse destination appends all the
 * lists or none (MSC_ERR_OOM). */
int msc_hist_copy_batch(msc_ctx* ctx, msc_hist_set* dst, const uint32_t* dst_slots, const msc_hist_set* src, const uint32_t* src_slots, uint64_t n);
/* msc_hist_clone for n slots in one launch per region: the Center(c->clone()) of every cluster the accumulate stage opened
 * (cluster/ClusterFactory.cpp:560-575, cluster/Center.h:13-40) -- a centre is not read before the update stage, so a driver may
 * queue its clones and issue them together. */
int msc_hist_clone_batch(msc_ctx* ctx, msc_hist_set* dst, const uint32_t* dst_slots, const msc_hist_set* src, const uint32_t* src_slots, uint64_t n);
/* The reverse complement of n slots, on the device: the histogram of a reverse-complemented sequence is a fixed permutation of the bins, so
 * the operator needs no sequence and applies to centres, means and uploaded bins alike. The reference has no counterpart: its users orient
 * their input by hand before fastcar's work() compares histograms as stored (fastcar/FC_Runner.cpp:426-471).
 * Index rule: A = 0, C = 1, G = 2, T = 3, a k-mer x0 .. x(k-1) has bin sum xi * 4^(k-1-i) (the order of msc_hist_download); rc(b) is the bin
 * whose digit of weight 4^j is 3 - (the digit of weight 4^(k-1-j) of b), an involution, and bins'[b] = bins[rc(b)]. The operator is DEFINED as
 * this permutation, not as a rebuild (for sequences of ACGT the two agree; the segment rules around runs of N are not mirror-symmetric).
 * Record rule: the scalar record is an exact copy, as msc_hist_copy_batch's (every word, a stale mag included -- sum, sum_sq, max_count,
 * overflow, length, n_kmers and stddev do not change under a permutation), except that one_mers is reversed (one_mers'[i] = one_mers[3 - i])
 * and a dense slot's tile prefixes follow the new bins. A sparse slot's list is mapped, sorted by the new bin and gets its cum and sub-range
 * table rebuilt: the slot the sparse builder writes for the reverse-complement sequence. Lists of more than 32 768 entries go through a dense
 * scratch slot, as the builder's long sequences do, with that route's limits (k <= 13).
 * Arguments as msc_hist_copy_batch: same ctx, k, dtype and layout; slots in range; destination slots distinct; n == 0 is MSC_OK; a sparse
 * destination appends all the lists or none (MSC_ERR_OOM). There is no in-place form: dst == src with a slot in both lists is
 * MSC_ERR_INVALID_ARG. Every mirror of the destination is rebuilt at its next use. msc_last_kernel_info names what ran ("k_hist_revcomp",
 * "k_sparse_revcomp_sort" or "k_sparse_revcomp_scratch", queries_per_candidate_read = 0). */
int msc_hist_revcomp_batch(msc_ctx* ctx, msc_hist_set* dst, const uint32_t* dst_slots, const msc_hist_set* src, const uint32_t* src_slots, uint64_t n);
/* The strand-neutral (canonical) form of n slots, on the device: every k-mer counted together with its reverse complement, so that a sequence and
 * its reverse complement become the SAME point and the mean-shift stages need not know about strands. The reference has no counterpart: fastcar's
 * work() compares histograms as stored (fastcar/FC_Runner.cpp:426-471), the loader counts the strand it is given (clutil/Loader.cpp:138-179), and
 * its users orient their input by hand. Like msc_hist_revcomp_batch the operator needs no sequence: centres, means and uploaded bins alike.
 * Definition: D is the slot as msc_hist_download returns it (natural order, the pseudocount of 1 in every bin), T the set's bin type, rc the index
 * rule stated at msc_hist_revcomp_batch:
 *     canon(D)[b] = clamp(D[b] + D[rc(b)] - 1, 0, max(T)),   the sum computed without wrap-around.
 * A k-mer counted c times forward and c' times in reverse holds 1 + c + c'; a palindromic bin (b == rc(b), even k only) holds 2 * D[b] - 1. The
 * result is symmetric under rc; a second application applies the formula again (it is not special-cased).
 * Record rule: length and id are copied from the source; one_mers'[i] = one_mers[i] + one_mers[3 - i] - 1; mag, sum, sum_sq, max_count, stddev and
 * a dense slot's tile prefixes are recomputed from the new bins, the bits msc_hist_upload gives for those bins (mag fresh, as after
 * msc_hist_clone); overflow' = the source's overflow OR some bin's exact sum exceeded max(T). The set's bounds (msc_hist_set_build_info) are
 * refreshed: a canonical slot can double them. A sparse slot's list is the merge by bin of the source's list and of its rc-mapped list, cum and
 * the sub-range table rebuilt: the slot the sparse builder would have written for those bins. Lists of more than 16 384 entries go through a
 * dense scratch slot, with that route's limits (k <= 13).
 * Arguments as msc_hist_copy_batch: same ctx, k, dtype and layout; slots in range; destination slots distinct; n == 0 is MSC_OK. A sparse
 * destination appends all the lists or none (MSC_ERR_OOM, the destination untouched); a canonical list has up to twice the source's entries.
 * Unlike the reverse complement there IS an in-place form: with dst == src, dst_slots[i] == src_slots[i] is legal for every i, and in-place and
 * out-of-place results are byte-identical. A slot that is the destination of one i and the source of a different i is MSC_ERR_INVALID_ARG. On a
 * sparse set the in-place form appends the new list and leaves the old one behind in the arena, as msc_hist_assign_batch does.
 * Every mirror of the destination is rebuilt at its next use. msc_last_kernel_info names what ran ("k_hist_canonical",
 * "k_sparse_canonical_sort" or "k_sparse_canonical_scratch", queries_per_candidate_read = 0). */
int msc_hist_canonical_batch(msc_ctx* ctx, msc_hist_set* dst, const uint32_t* dst_slots, const msc_hist_set* src, const uint32_t* src_slots, uint64_t n);

/* ------------------------------------------------------------------ a5/a7: model (Feature<T> + GLM weights) */
/* Mirrors the state Predictor::read_from builds (predict/Predictor.cpp:125-185): combos are replayed through
 * Feature::add_feature (predict/Feature.cpp:102-128) so single-feature order == order of first appearance.
 *   combo_kind[c] in MSC_COMBO_*, combo_flags[c] = OR of its 1-2 single bits, weights[0] = intercept.
 *   single_flags/mins/maxs: the n_singles lines of the file (any order).
 *   bias: Predictor::set_bias global (predict/Predictor.cpp:307-313), default 0. */
int  msc_model_create(msc_ctx* ctx, int k, int n_combos, const int* combo_kind, const uint64_t* combo_flags,
                      const double* weights, int n_singles, const uint64_t* single_flags, const double* mins,
                      const double* maxs, double bias, msc_model** out);
/* Reads a `--dump` / weights.txt file (predict/Predictor.cpp:28-44,47-121). block 0 = classification, 1 = regression. */
int  msc_model_load(msc_ctx* ctx, const char* path, int block, msc_model** out);
int  msc_model_parse(msc_ctx* ctx, const char* text, int block, msc_model** out);
void msc_model_destroy(msc_model* m);
int  msc_model_k(const msc_model* m);
int  msc_model_n_singles(const msc_model* m);
int  msc_model_n_combos(const msc_model* m);
int  msc_model_single_flags(const msc_model* m, uint64_t* flags_out /* n_singles */);
void msc_model_set_bias(msc_model* m, double bias);

/* ------------------------------------------------------------------ a5/a6: pair scoring, 1 query x m candidates */
/* Raw statistics (predict/Feature.cpp, the 11 functions of SURVEY 8a-a6) of (cands[cand_slots[i]], q) for every
 * bit in feat_mask. raw_out is m x popcount(feat_mask), row i = candidate i, columns in ascending bit order.
 * Replaces Feature<T>::<raw fn> call sites predict/Feature.cpp:156-171 and FeatureSelector's table
 * (predict/FeatureSelector.cpp:23-33). cand_slots == NULL means slots 0..m-1. */
int msc_pair_features_raw(msc_ctx* ctx, const msc_hist_set* cands, const uint32_t* cand_slots, uint64_t m,
                          const msc_hist_set* qset, uint64_t q_slot, int order, uint64_t feat_mask, double* raw_out);

/* Feature::compute + operator() + weighted sum (predict/Feature.h:197-239; cluster/Trainer.cpp:112-120;
 * predict/Predictor.cpp:284-333). Any output pointer may be NULL.
 *   singles_out : m x n_singles normalised values (the `cache` vector)
 *   combos_out  : m x n_combos
 *   sum_out     : m, s = w0 + sum_c w_c * combo_c
 *   csum_out    : m, classify_sum = logistic(s) + bias
 * Rows of candidates for which the reference would throw hold NaN and the call returns MSC_ERR_ZERO_LENGTH/NAN. */
int msc_score(msc_ctx* ctx, const msc_model* model, const msc_hist_set* cands, const uint32_t* cand_slots, uint64_t m,
              const msc_hist_set* qset, uint64_t q_slot, int order,
              double* singles_out, double* combos_out, double* sum_out, double* csum_out);

/* n_q queries x m candidates in ONE pass over the candidates (the all-pairs shape: fastcar work(),
 * fastcar/FC_Runner.cpp:426-471; the training table, predict/FeatureSelector.cpp:23-33). Every candidate tile read from
 * HBM is scored against several query tiles held in registers. Outputs are query-major: [n_q][m] (raw_out
 * [n_q][m][popcount(feat_mask)]). Any output pointer may be NULL; model may be NULL when only raw_out is wanted.
 * close_out[q][i] = round(classify_sum) > 0. */
int msc_score_multi(msc_ctx* ctx, const msc_model* model, const msc_hist_set* cands, const uint32_t* cand_slots, uint64_t m,
                    const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q, int order,
                    double* sum_out, double* csum_out, uint8_t* close_out, uint64_t feat_mask, double* raw_out);
/* counts[q] = number of close candidates of query q in the last msc_score_multi call that asked for close_out (the row sums of
 * close_out, added up on the device: the per-query result of fastcar's work() loop, fastcar/FC_Runner.cpp:449-455, without a host pass
 * over n_q x m flags). MSC_ERR_UNSUPPORTED when that call took a route that keeps no counts (one pass per query). */
int msc_last_close_counts(msc_ctx* ctx, uint64_t* counts, uint64_t n_q);

/* An explicit list of n pairs (a_i, b_i) scored in one pass: the shape of the reference's feature table, which walks a
 * vector<pair<Point*, Point*>> (predict/FeatureSelector.cpp:23-33; the table both trainers start from, predict/Predictor.cpp:876-985), and of
 * any caller that wants the statistics or the score of chosen pairs (every member to its centre, a model checked on labelled pairs,
 * candidate pairs of another tool) without one 1 x 1 pass per pair.
 *   Row i of every output is what msc_pair_features_raw / msc_score give for the single-candidate call (m = 1, same order, same feat_mask /
 *   model) with candidate = slot a_slots[i] of a_set and query = slot b_slots[i] of b_set; close_out[i] = round(classify_sum) > 0 as in
 *   msc_score_multi. Rows come back in the caller's order. Repeated pairs, a_set == b_set and a_slots[i] == b_slots[i] are legal.
 *   a_slots == NULL or b_slots == NULL means slots 0 .. n-1. raw_out is n x popcount(feat_mask), columns in ascending bit order (feat_mask
 *   is read only with raw_out); singles_out n x n_singles, combos_out n x n_combos, sum_out / csum_out / close_out n. Any output pointer
 *   may be NULL, model may be NULL when only raw_out is wanted; all outputs NULL is MSC_ERR_INVALID_ARG; n == 0 is MSC_OK.
 *   Argument checks are those of msc_score: the ctx owns both sets and the model, the sets agree in k, dtype and layout (one dense and one
 *   sparse set are refused, as by every 1 x M call), slots in range; and the model's k is the sets'. A row for which the reference would
 *   throw holds NaN and the call returns MSC_ERR_ZERO_LENGTH / MSC_ERR_NAN as msc_score does; the other rows are still filled. There is
 *   no length window.
 * Which values share bits with the per-pair calls: every statistic other than jefferey_divergence / jensen_shannon is a closed form of exact
 * integer reductions and the slots' scalars, evaluated by the one epilogue, so those columns -- and singles / combos / sum / csum / close of
 * a model that holds no divergence statistic -- are bit-equal to msc_pair_features_raw / msc_score per pair on every route. The two
 * divergence sums come from the pair-list form of the chunked merge kernel only, so they are bit-equal to the routes DESIGN.md 4.6 lists as
 * sharing bits (msc_score_multi's raw_out is one of them), whatever the order of the list or the way it is cut into calls; where that
 * kernel does not apply the call goes query by query through the 1 x M calls, so nothing new is introduced there.
 * The pairs are grouped by b slot; msc_last_kernel_info names the pass kernel (queries_per_candidate_read = 1): "k_pair_sparse_wl_pairs"
 * (two sparse sets, or dense sets of histograms >= 64 KiB through their mirrors; 32-bit range; the two sets' longest lists fit a wave's
 * LDS region together; integer statistics), "k_pair_sparse_mp" (the same with longer lists, or with a divergence statistic),
 * "k_pair_tiles_batch" (dense sets without a list form, narrow range, no divergence statistic), or -- the wide range, sparse counts >=
 * 2^16, MSC_FEAT_GROUPS, a divergence statistic the chunked merge kernel would not serve -- one 1 x M call per distinct b slot, reported as
 * that call's kernel name followed by " per query". */
int msc_score_pair_list(msc_ctx* ctx, const msc_model* model,
                        const msc_hist_set* a_set, const uint32_t* a_slots,
                        const msc_hist_set* b_set, const uint32_t* b_slots, uint64_t n, int order,
                        uint64_t feat_mask, double* raw_out,
                        double* singles_out, double* combos_out, double* sum_out, double* csum_out, uint8_t* close_out);

/* ------------------------------------------------------------------ the quantity every model here predicts: global-alignment identity
 * Feature::align (predict/Feature.cpp:697-718, FEAT_ALIGN) over utility/GlobAlignE.cpp:123-292, for n_pairs listed pairs in one call: an
 * affine-gap global alignment WITHOUT traceback whose every state carries its score, the alignment length so far and the identical columns
 * so far. All integers, every tie in a fixed order: the triple (score, length, matches) is the reference's, bit for bit; identity =
 * (double)matches / length is left to the caller. DESIGN.md 4.6e restates the recurrence.
 *   sequence s = seqs[offsets[s] .. offsets[s+1]), host memory; pair p = (first[p], second[p]), first is GlobAlignE's seq1. Ties are NOT
 *   symmetric in the two sequences: no pair is reordered, and both orders of a pair may differ. Bytes are compared for equality and nothing
 *   else: no alphabet, no case folding, an N equals an N. A pair of a sequence with itself and repeated pairs are legal.
 *   match, mismatch, gap_open, gap_continue: Feature::align passes 1, -1, 2, 1 (a gap of g columns costs gap_open + g * gap_continue).
 *   The reference's finite stand-in for minus infinity ([-gap_open - |la - lb| * gap_continue, only if la != lb] + mismatch * min(la, lb) - 1),
 *   its boundary row and column and its tie orders are reproduced as written; no banding, no approximation.
 *   score / length / matches: n_pairs each, host memory, the caller's order.
 * Checked on the host before anything is queued, MSC_ERR_INVALID_ARG with every output untouched otherwise: every LISTED sequence has
 * 1 .. 32 767 bytes, the four parameters are at most 100 in absolute value, indices are below n_seqs. n_pairs == 0 is MSC_OK.
 * One pair per wave, the anti-diagonals as a systolic array over the lanes; pairs are dealt longest first; the sequences are uploaded once per
 * call. msc_last_kernel_info names the kernel, "k_align_pairs<carry in LDS>" or "k_align_pairs<carry in global memory>" (that of the call's
 * last launch; queries_per_candidate_read = 0). Results do not depend on the order of the list, on the other pairs of a call or on the
 * context's history. */
int msc_align_pairs(msc_ctx* ctx,
                    const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                    const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                    int match, int mismatch, int gap_open, int gap_continue,
                    int32_t* score, int32_t* length, int32_t* matches);

/* ------------------------------------------------------------------ the same integers over a band of diagonals, with a proof per pair
 * For SIMILAR pairs (the hits of msc_fastcar --align, a cluster's members against its centre) the optimal path stays near the corner-to-corner
 * line, and filling the whole grid is wasted work. Both calls below take the lists, the parameters, the limits and the refusals of
 * msc_align_pairs (1 .. 32 767 bytes, parameters at most 100 in absolute value, indices below n_seqs, MSC_ERR_INVALID_ARG with every output
 * untouched otherwise, n_pairs == 0 is MSC_OK, results in the caller's order). DESIGN.md 4.6f has the definition and the proof.
 *
 * msc_align_pairs_banded: the recurrence over the diagonals min(0, la - lb) - band .. max(0, la - lb) + band of the grid only (cell (i, j)
 *   lies on diagonal i - j); every state outside them is the constant (-2^30, 0). Any uint32 is a legal band; one of min(la, lb) or more
 *   covers the grid. The triple is a function of (pair, parameters, band) alone, certified or not.
 *   certified[p] = 1: the pair's triple is PROVEN to be msc_align_pairs's, bit for bit -- by an integer test on the banded score (it exceeds
 *   every score a path through a cell outside the band can reach), or because the band covers the grid. 0: not proven; the triple may or may
 *   not be the full one. The test is offered only where gap_open >= 0, gap_continue >= 0 and max(match, mismatch) + 2 * gap_continue >= 0;
 *   under other parameters only a covering band certifies.
 * msc_align_pairs_auto: msc_align_pairs's triples, always and under every parameter set, with fewer cells filled for similar pairs. Every
 *   pair starts at first_band (0: the library's default, 64) and is rerun with its band doubled while it is not certified; a pair whose
 *   band's row window (diagonals + 64 * columns a lane - 1 rows) would exceed half of its rows, and every pair under parameters without a
 *   certificate, goes through k_align_pairs instead. band_used (may be NULL): the band that certified pair p, 0xffffffff where the full
 *   kernel ran. Worth it from about 1 000 bytes a sequence at 97 % identity and from 5 000 bytes at 85 - 95 % (profiles/align_band.md);
 *   below that it costs what msc_align_pairs costs, plus a round that certified nothing.
 * One pair per wave, the systolic sweep of k_align_pairs over the rows each stripe of columns has in band; the sequences are uploaded once
 * per call, each round of msc_align_pairs_auto launches only the pairs still open, each at its own band. msc_last_kernel_info names
 * "k_align_band<C column(s) a lane, carry in LDS | global memory>" (of the call's last banded launch; k_align_pairs's name where
 * msc_align_pairs_auto ran no banded round). */
int msc_align_pairs_banded(msc_ctx* ctx,
                           const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                           const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                           int match, int mismatch, int gap_open, int gap_continue, uint32_t band,
                           int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified);
int msc_align_pairs_auto(msc_ctx* ctx,
                         const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                         const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                         int match, int mismatch, int gap_open, int gap_continue, uint32_t first_band,
                         int32_t* score, int32_t* length, int32_t* matches, uint32_t* band_used);

/* ------------------------------------------------------------------ the same three calls for LONG sequences
 * msc_align_pairs_long, msc_align_pairs_long_banded and msc_align_pairs_long_auto take the arguments of their namesakes above and return
 * what they return -- the same recurrence, boundaries, finite "minus infinity" and tie orders, the same band, out-of-band constant -2^30 and
 * certificate, `first` is sequence 1, int32 score, length and matches -- for listed sequences of 1 .. 1 048 575 bytes (kAlignLongMaxLen,
 * 2^20 - 1: every score the recurrence forms stays inside int32 and every real score above anything derived from -2^30, proven in 4.6g).
 * Parameters are at most 100 in absolute value; the other checks are msc_align_pairs's, made before anything is queued; a refusal returns
 * MSC_ERR_INVALID_ARG with every output untouched; n_pairs == 0 is MSC_OK. The three calls above keep their limit of 32 767 bytes.
 *   A pair with both sequences within 32 767 bytes goes through the queueing of the calls above, so through k_align_pairs / k_align_band<>,
 *   and comes out bit for bit as from them. Every other pair is cut into tiles of 256 columns by H rows (256; MSC_ALIGN_TILE_ROWS=n) that
 *   k_align_tiles fills one wave a tile, launch after launch along the anti-diagonals of the tile grid, with states whose length and count have
 *   a word each; MSC_ALIGN_LONG_ALL=1 sends every pair there. Both switches are read on every call. Results come back in the caller's order.
 *   msc_align_pairs_long_auto: first_band (0: the library's default, 64), doubled per uncertified pair, one group of launches a round; a
 *   pair that a band no longer helps goes to the full grid; band_used (may be NULL) as above, 0xffffffff for the full grid.
 * msc_last_kernel_info names "k_align_tiles<wide states, H rows a tile>" whenever one of its launches ran in the call, otherwise what the
 * namesake would name. */
int msc_align_pairs_long(msc_ctx* ctx,
                         const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                         const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                         int match, int mismatch, int gap_open, int gap_continue,
                         int32_t* score, int32_t* length, int32_t* matches);
int msc_align_pairs_long_banded(msc_ctx* ctx,
                                const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                                const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                int match, int mismatch, int gap_open, int gap_continue, uint32_t band,
                                int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified);
int msc_align_pairs_long_auto(msc_ctx* ctx,
                              const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                              const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                              int match, int mismatch, int gap_open, int gap_continue, uint32_t first_band,
                              int32_t* score, int32_t* length, int32_t* matches, uint32_t* band_used);

/* ------------------------------------------------------------------ the alignment itself: a CIGAR per pair
 * msc_align_pairs_trace takes the lists, the parameters, the limits and the refusals of msc_align_pairs (sequences of 1 .. 32 767 bytes,
 * parameters at most 100 in absolute value, indices below n_seqs, checked before anything is queued: MSC_ERR_INVALID_ARG with every output
 * untouched; n_pairs == 0 is MSC_OK, with op_offsets[0] = 0 where the pointer is given) and returns msc_align_pairs's triples, bit for bit,
 * together with the path they were counted along.
 *   The path is a function of (pair, parameters) alone: it starts at the corner (la, lb) in the state the result's maximum picks (match, then
 *   lower, then upper) and follows the winners of the recurrence back, with its tie orders -- a match state leaves a diagonal column and goes
 *   to the state that won its maximum; a lower (upper) state leaves a column that consumes a byte of sequence 1 (2) and goes to match where
 *   the gap opened, else stays -- until it reaches row 0 or column 0, where the i (j) columns left consume sequence 1 (2).
 *   Encoding: the columns in forward order, run-length encoded, one uint32 per run, run << 4 | op, with BAM's op numbers; `first`
 *   (sequence 1, msc_fastcar's query) is the query and `second` the reference: 7 '=' a diagonal column whose bytes are equal, 8 'X' one
 *   whose bytes differ, 1 'I' a column that consumes sequence 1 only, 2 'D' one that consumes sequence 2 only. Adjacent runs never share an op.
 *   op_offsets: n_pairs + 1 words, host memory; pair p's runs are words op_offsets[p] .. op_offsets[p + 1] of the list, the caller's order.
 *   The list stays on the device until the next msc_align_pairs_trace on ctx or msc_destroy; msc_align_pairs_trace_fetch copies words
 *   first_word .. first_word + n_words of it to host memory; a range past its end is MSC_ERR_INVALID_ARG.
 * Invariants (proven in 4.6h): (1) the columns of a pair's runs number `length`, under every parameter set; (2) its '=' columns
 * number `matches` whenever match != mismatch (with match == mismatch the reference counts every diagonal column); (3) where the walk ends on a
 * boundary state that is not the reference's finite "minus infinity" (a REAL path: every related pair), the affine score of the runs -- match
 * or mismatch per diagonal column, -(gap_open + g * gap_continue) per gap run of g columns -- is `score`. For the other paths only (1) and
 * (2) are promised.
 * k_align_pairs's schedule with one 16-bit word of back pointers stored per lane and step (4 bits a cell: ceil(la / 256) * (lb + 63) * 128
 * bytes a pair), then one lane per pair walks them twice: to count the runs and, behind a scan, to write them. The pairs are dealt in the
 * caller's order into groups whose back pointers fit 2 GiB (kAlignTraceBytes; MSC_ALIGN_TRACE_BYTES=n overrides it, read on every call; a pair
 * above the cap is a group of its own); results do not depend on the grouping, the order of the list, the other pairs or the context's
 * history. msc_last_kernel_info names "k_align_pairs_dirs<carry in LDS>" or "k_align_pairs_dirs<carry in global memory>" (of the call's last
 * forward launch); msc_last_kernel_ms gives the forward launches (tiles_ms) and the call's whole span on the device. Banded and long
 * (> 32 767 bytes) traceback are not offered. */
int msc_align_pairs_trace(msc_ctx* ctx,
                          const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                          const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                          int match, int mismatch, int gap_open, int gap_continue,
                          int32_t* score, int32_t* length, int32_t* matches, uint64_t* op_offsets);
int msc_align_pairs_trace_fetch(msc_ctx* ctx, uint64_t first_word, uint64_t n_words, uint32_t* ops);

/* ------------------------------------------------------------------ a8/a9: Trainer operators */
/* Trainer<T>::get_close (cluster/Trainer.cpp:23-71; caller cluster/ClusterFactory.cpp:566).
 * The window [istart, iend) is cand_slots[0..m). Candidates outside floor(len_q*cutoff) <= len <= floor(len_q/cutoff)
 * are skipped. close_flags[i] = 1 where the reference sets (*i).second = true. best_pos = index INTO cand_slots of the
 * arg-max of combo 0 (first maximum in window order = OMP_NUM_THREADS=1 order), -1 if nothing passed the length
 * filter (then best_sim = -1). is_min = no candidate was close. `cutoff` is Trainer::cutoff as given (not get_id()). */
int msc_get_close(msc_ctx* ctx, const msc_model* model, double cutoff,
                  const msc_hist_set* cands, const uint32_t* cand_slots, uint64_t m,
                  const msc_hist_set* qset, uint64_t q_slot,
                  uint8_t* close_flags, int64_t* best_pos, double* best_sim, int* is_min);

/* Trainer<T>::filter (cluster/Trainer.cpp:123-141; caller cluster/ClusterFactory.cpp:312): keep[i] = 1 iff point i
 * is inside the length window of the centre (get_id() form of cutoff) AND round(classify(centre, point)) != 0. */
int msc_filter(msc_ctx* ctx, const msc_model* model, double cutoff,
               const msc_hist_set* centre_set, uint64_t centre_slot,
               const msc_hist_set* pts, const uint32_t* pt_slots, uint64_t m, uint8_t* keep, uint64_t* n_kept);

/* Trainer<T>::merge (cluster/Trainer.cpp:74-109; caller cluster/ClusterFactory.cpp:387): among centres
 * centre_slots[begin..last] inside the length window of centre_slots[current] with round(classify_sum) == 1,
 * the index with the largest combo 0 (later index wins ties; initial best (0, DBL_MIN)). */
int msc_merge(msc_ctx* ctx, const msc_model* model, double cutoff,
              const msc_hist_set* centres, const uint32_t* centre_slots, uint64_t n,
              int64_t current, int64_t begin, int64_t last, int64_t* best_out);

/* Predictor::close + similarity for one query against m database entries (fastcar/FC_Runner.cpp:426-471 work()):
 * close_out[i] = p_close (classification block), sim_out[i] = p_predict (regression block, clamped to [0,1]).
 * work() follows Predictor::get_mode() (:432,446-458): cls == NULL (a `mode: 2` weights file) makes every entry close,
 * reg == NULL (a `mode: 1` file, what `meshclust2 --dump` writes) makes every similarity 1. Not both NULL. */
int msc_search(msc_ctx* ctx, const msc_model* cls, const msc_model* reg,
               const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
               const msc_hist_set* qset, uint64_t q_slot, uint8_t* close_out, double* sim_out);

/* fastcar's work() (fastcar/FC_Runner.cpp:426-471) for n_q queries against one candidate list, with only the CLOSE pairs as output: what a
 * search asks (which pairs are close, and their identity) at a size that follows the close pairs instead of n_q x m.
 * Pair (q, i) is listed iff win_lo[q] <= i < win_hi[q] (both NULL: every i < m; win_hi is clamped to m) and, when cls != NULL,
 * p_close(db[db_slots[i]], query q) (MSC_ORDER_CAND_FIRST, as msc_search). Its similarity is clamp(p_predict, 0, 1) with reg, 1 without
 * it -- bit for bit what msc_search gives for that pair; pairs of similarity 0 are listed too. cls == reg == NULL is MSC_ERR_INVALID_ARG.
 * Pairs are ordered by query, then by ascending i. offsets[n_q + 1] is filled on return (offsets[0] = 0; query q's pairs are
 * [offsets[q], offsets[q + 1])). The pairs of each block of queries are evaluated over the union of its members' windows, so the error
 * statuses (zero length, NaN) are those msc_score_multi returns for those pairs. The list stays on the device until the next
 * msc_search_pairs call on ctx or msc_destroy; msc_search_pairs_fetch copies a range of it (either output may be NULL).
 * info (nullable): n_pairs; route = MSC_PAIRS_ROUTE_MATRIX when the product on the matrix cores served the call (dense sets -- with
 * msc_set_sparse_matrix_pass two sparse sets as well -- of whole 4 KiB tiles, n_q >= 2, no divergence or group statistic in either
 * model), MSC_PAIRS_ROUTE_FALLBACK when msc_score_multi's other routes did, one block of queries at a time; fp64_pairs = pairs evaluated
 * in FP64 (regression evaluations plus classification pairs the f32 screen left undecided, or every classification pair where there is
 * no screen). */
#define MSC_PAIRS_ROUTE_MATRIX   1
#define MSC_PAIRS_ROUTE_FALLBACK 2
typedef struct {
	uint64_t n_pairs;
	int32_t  route;
	int32_t  pad_;
	uint64_t fp64_pairs;
} msc_pairs_info;
int msc_search_pairs(msc_ctx* ctx, const msc_model* cls, const msc_model* reg,
                     const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
                     const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q,
                     const uint64_t* win_lo, const uint64_t* win_hi, uint64_t* offsets, msc_pairs_info* info);
int msc_search_pairs_fetch(msc_ctx* ctx, uint64_t first, uint64_t n, uint32_t* cand_idx, double* sim);

/* msc_search_pairs with each query's list cut to its top_n best pairs on the device: the loop whose output is cut is fastcar's work()
 * (fastcar/FC_Runner.cpp:426-471). Let S_q be the pairs msc_search_pairs lists for query q (same windows, models and similarities).
 * With top_n > 0 the call lists all of S_q when |S_q| <= top_n, and otherwise the top_n pairs of S_q with the largest similarity:
 * similarities are compared as doubles (-0.0 == 0.0), ties go to the lower candidate index i, the kept pairs stay in ascending i (the
 * result is a subsequence of the full list) and their similarities are the bits the full list holds. Pairs of similarity 0 take part
 * like any other: they are the smallest, so they are kept only where fewer than top_n pairs are positive. top_n == 0 means no cut: the
 * result is msc_search_pairs's. There is no upper limit on top_n.
 * Argument checks, error statuses, the route, info->route and info->fp64_pairs are msc_search_pairs's; offsets and info->n_pairs describe
 * the kept list, which msc_search_pairs_fetch reads; close_counts (nullable, [n_q]) receives |S_q|, the pairs before the cut. The
 * selection runs on the device block by block of queries: the list never holds more than the kept pairs, and one block's uncut pairs
 * lie beside it in a staging list. */
int msc_search_pairs_top(msc_ctx* ctx, const msc_model* cls, const msc_model* reg,
                         const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
                         const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q,
                         const uint64_t* win_lo, const uint64_t* win_hi, uint32_t top_n,
                         uint64_t* offsets, uint64_t* close_counts, msc_pairs_info* info);

/* msc_search_pairs on both strands: fastcar's work() (fastcar/FC_Runner.cpp:426-471) compares a query with a database entry as stored, so a
 * read that is the reverse complement of an entry is an unrelated histogram to it, and the reference's users orient their input by hand.
 * Let F be the list msc_search_pairs gives for these arguments and R the list it gives when every query is replaced by its reverse
 * complement (msc_hist_revcomp_batch: bins'[b] = bins[rc(b)], rc(b) = the bin whose digit of weight 4^j is 3 - (the digit of weight
 * 4^(k-1-j) of b); the record copied with one_mers reversed), same windows. The candidates are never permuted: the earth mover's distance
 * depends on the bin order, so "the query's reverse complement against the stored candidate" is the definition.
 * Merge rule, per query: the union of F_q and R_q over the candidate index i, ascending in i. A pair of one list keeps that list's similarity
 * bits and gets strand 0 (forward) or 1 (reverse); a pair of both keeps the larger similarity, compared as doubles, and a tie goes to forward.
 * offsets, msc_search_pairs_fetch (idx, sim) and msc_search_pairs_fetch_strands (one byte per pair) read the merged list;
 * msc_search_pairs_fetch_strands after a search that was not this one is MSC_ERR_UNSUPPORTED.
 * info: n_pairs = the merged count, fp64_pairs = the sum of both passes, route = MSC_PAIRS_ROUTE_MATRIX iff both passes report it (the reverse
 * complements inherit the queries' bounds, so both take the same route). Argument checks and error statuses are msc_search_pairs's; n_q == 1
 * is legal, m == 0 and n_q == 0 are MSC_OK with empty lists.
 * Scratch size: the reverse complements live in a set of n_q slots of the query set's k, dtype and layout that the context owns (a sparse one
 * with an arena of the queries' stored bins), reused and grown between calls and freed by msc_destroy; no device memory for it is MSC_ERR_OOM
 * with the byte count in msc_last_error. A dense slot is 4^k * sizeof(T) bytes: the caller batches its queries where n_q slots matter. */
int msc_search_pairs_strands(msc_ctx* ctx, const msc_model* cls, const msc_model* reg,
                             const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
                             const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q,
                             const uint64_t* win_lo, const uint64_t* win_hi, uint64_t* offsets, msc_pairs_info* info);
int msc_search_pairs_fetch_strands(msc_ctx* ctx, uint64_t first, uint64_t n, uint8_t* strand);

/* ------------------------------------------------------------------ a8 over a device-resident window
 * The accumulate loop (cluster/ClusterFactory.cpp:553-610) hands Trainer::get_close an iterator range of the length-sorted store
 * (bvec::get_range, cluster/bvec.cpp:261-330; the loop `for (i = istart; i < iend; ++i)` of cluster/Trainer.cpp:41-48). A
 * msc_window keeps that store's ORDER on the device: position i holds slot slots[i] of `set` and an alive flag, all alive at first.
 * A step then passes the positions [first, end) instead of a slot list rebuilt on the host: host work per step is O(close).
 *   msc_get_close_window: get_close over the ALIVE positions of [first, end) in position order; same window rule, arg-max and
 *     tie order as msc_get_close. *close_pos (valid until the next call on this window) lists the n_close positions the reference
 *     would mark, ascending; they DIE with the call -- the loop removes marked points next (remove_available,
 *     cluster/ClusterFactory.cpp:598). best_pos = POSITION of the arg-max, -1 if nothing passed the length filter.
 *   msc_window_kill: positions that leave the store otherwise (bvec::erase of the next seed :589, bvec::pop :593).
 *   msc_window_alive: alive positions in [first, end), from the host-side count the library keeps (no device read-back).
 *   msc_window_last_compaction: the grid of the compaction launch of the last msc_get_close_window on this window -- (1, 1024): one
 *     workgroup; (n, 256) / (n, 1024): the multi-block form; (0, 0): the call returned before launching (nothing alive in the range).
 *   msc_window_last_close_blocks: the workgroups of the close pass that call launched as a kernel of its own; 0 where the pass rode in
 *     the fused epilogue + reduce kernel (the default for histograms of up to four tiles) or the call returned early. Both are host
 *     bookkeeping for tests: they tell which form of a step ran, and read no device memory. */
typedef struct msc_window msc_window;
int      msc_window_create(msc_ctx* ctx, const msc_hist_set* set, const uint32_t* slots, uint64_t n, msc_window** out);
void     msc_window_destroy(msc_window* w);
uint64_t msc_window_alive(const msc_window* w, uint64_t first, uint64_t end);
int      msc_window_kill(msc_ctx* ctx, msc_window* w, const uint32_t* positions, uint64_t n);
void     msc_window_last_compaction(const msc_window* w, uint32_t* blocks, uint32_t* threads);
uint32_t msc_window_last_close_blocks(const msc_window* w);
int      msc_get_close_window(msc_ctx* ctx, const msc_model* model, double cutoff, msc_window* w, uint64_t first, uint64_t end,
                              const msc_hist_set* qset, uint64_t q_slot, const uint32_t** close_pos, uint64_t* n_close,
                              int64_t* best_pos, double* best_sim, int* is_min);

/* ------------------------------------------------------------------ a4/a10: mean-shift metric */
/* get_mean (cluster/ClusterFactory.cpp:338-380), the mean part of mean_shift_update (:297-326) and Trainer::closest
 * (cluster/Trainer.cpp:144-157): FP64 column mean of the m members, DivergencePoint::distance_d
 * (clutil/DivergencePoint.cpp:55-66) of every member to it, first arg-min.
 * dist_out (m) and mean_out (4^k doubles, natural order) may be NULL. */
int msc_mean_nearest(msc_ctx* ctx, const msc_hist_set* set, const uint32_t* member_slots, uint64_t m,
                     int64_t* nearest_pos, double* dist_out, double* mean_out);

/* The whole update stage of one mean-shift round in three launches: for centre c (slot centre_slots[c] of `centres`) and its
 * neighbourhood list pt_slots[offsets[c] .. offsets[c+1]) of `pts`: Trainer::filter, the FP64 mean of the survivors and
 * the survivor nearest that mean -- mean_shift_update, cluster/ClusterFactory.cpp:288-335, which the reference runs for all
 * centres of a round under `omp parallel for` (:639). nearest_pos[c] = position INSIDE centre c's list of the new centre
 * point, or -1 when nothing survives the filter; n_kept[c] (nullable) = survivors. Same results as msc_filter followed by
 * msc_mean_nearest per centre (which is also what runs for divergence / group statistics, the wide range, and sparse sets with
 * counts >= 2^16; sparse sets in the 32-bit range are batched too since r02). */
int msc_update_centres(msc_ctx* ctx, const msc_model* model, double cutoff, const msc_hist_set* centres, const uint32_t* centre_slots,
                       uint64_t n_centres, const msc_hist_set* pts, const uint32_t* pt_slots, const uint64_t* offsets, int64_t* nearest_pos,
                       uint64_t* n_kept);

/* Every Trainer::merge call of the serial merge loop (cluster/ClusterFactory.cpp:383-401: centre i against centres i+1 ..
 * min(n-1, i+delta), i = 0 .. n-1) in one launch; best_out[i] = what msc_merge returns for (current = i, begin = i + 1,
 * last = min(n - 1, i + delta)). No merge call changes a histogram, so the calls are independent. */
int msc_merge_all(msc_ctx* ctx, const msc_model* model, double cutoff, const msc_hist_set* centres, const uint32_t* centre_slots, uint64_t n,
                  int delta, int64_t* best_out);

/* ... for SOME of those calls: best_out[w] = what msc_merge returns for (current = which[w], begin = which[w] + 1,
 * last = min(n - 1, which[w] + delta)) over the same list of n centres. Once the clusters have settled a round of the merge loop
 * repeats the round before it; the driver asks only about the centres whose delta + 1 histograms changed. */
int msc_merge_some(msc_ctx* ctx, const msc_model* model, double cutoff, const msc_hist_set* centres, const uint32_t* centre_slots, uint64_t n,
                   int delta, const uint64_t* which, uint64_t n_which, int64_t* best_out);

/* ------------------------------------------------------------------ f2: training on labelled pairs
 * Replaces the feature-selection half of Predictor<T>::train (predict/Predictor.cpp:876-975): calculate_table,
 * BestFirstSelector<T>::train_class and GLM::train (predict/BestFirstSelector.cpp:113-250, predict/GLM.cpp:20-23) on pairs
 * (first_slots[i], second_slots[i]) of `pts` labelled vals[i] (identity in the unit of `id`); the first n_train pairs are the
 * training set, the next n_test the testing set. feat_flags = the single statistics on offer (MSC_FEAT_FAST / MSC_FEAT_SLOW).
 * The raw statistics come from the streaming kernels; selection and least squares are host work in the reference's evaluation
 * order. text_out receives a complete weights file (Predictor::save, :28-44) that msc_model_parse accepts. The reference's own
 * generation of the pairs (mutated templates, :519-710) is out of scope. */
int msc_train_class(msc_ctx* ctx, const msc_hist_set* pts, const uint32_t* first_slots, const uint32_t* second_slots, const double* vals,
                    uint64_t n_train, uint64_t n_test, uint64_t feat_flags, int min_feat, int max_feat, double id, char* text_out, size_t cap,
                    double* train_acc, double* test_acc);

/* The regression half of Predictor<T>::train (predict/Predictor.cpp:977-985 train_regr -> GreedySelector<T>::train_regression,
 * predict/GreedySelector.cpp:11-76): the model fastcar's work() reads identities from (Predictor::similarity -> p_predict, :284-300).
 * Same inputs as msc_train_class; vals are the identity labels the least-squares fit predicts. Greedy forward selection over the
 * candidates of Predictor::add_feats: at most max_feat rounds, a round keeps the candidate with the smallest mean absolute error over the
 * TESTING pairs if that beats every earlier round. text_out: a complete weights file with `mode: 2` (msc_model_parse(text, 1) reads
 * the block); train_err / test_err: mean |prediction - label| of the final fit. The reference's own function cannot run to its end
 * (no return statement: `fastcar --dump` dies there); oracle/ref_harness.cpp follows its body on the reference's objects and
 * tests/golden/train_regr_*.json holds the result. */
int msc_train_regr(msc_ctx* ctx, const msc_hist_set* pts, const uint32_t* first_slots, const uint32_t* second_slots, const double* vals,
                   uint64_t n_train, uint64_t n_test, uint64_t feat_flags, int max_feat, double id, char* text_out, size_t cap,
                   double* train_err, double* test_err);

/* ------------------------------------------------------------------ multi-GPU plumbing
 * Raw device views so that a caller that owns an RCCL communicator (torch.distributed / rccl.h) can broadcast a
 * query or all-gather centroid histograms between the per-GPU processes without a host bounce.
 *   slot_bytes  : bytes of one slot's bins region; slot i starts at bins + i*slot_bytes
 *   scalar_bytes: bytes of one slot's scalar record; slot i at scalars + i*scalar_bytes
 * After writing a slot's two regions from a peer's copy, call msc_hist_import_done() for those slots. */
int msc_hist_set_device_view(const msc_hist_set* set, void** bins, uint64_t* slot_bytes,
                             void** scalars, uint64_t* scalar_bytes);
int msc_hist_import_done(msc_ctx* ctx, msc_hist_set* set, uint64_t first_slot, uint64_t n);

/* A slot as ONE contiguous byte range in device memory, dense or sparse (scalar record + bins, or scalar record + sub-range table +
 * (bin, value) list + cum array: ~12 bytes per distinct k-mer instead of 4^k bins): what a sharded driver broadcasts as the query of
 * a Trainer::get_close step (cluster/ClusterFactory.cpp:566) and all-gathers as the new centres of an update round (:328,331).
 *   msc_hist_packed_bytes: size of slot's range (a multiple of 16; known on the host).
 *   msc_hist_pack:   slots[i] -> dev_dst + offsets[i] (offsets: multiples of 16, ranges disjoint).
 *   msc_hist_unpack: dev_src + offsets[i] -> slots[i] of `set` (same k, bin type and layout: the packed head records them,
 *                    MSC_ERR_INVALID_ARG otherwise), an exact copy -- stale magnitude
 *                    included; clone / assign semantics come from msc_hist_clone / msc_hist_assign(_batch) out of a staging set. A
 *                    sparse destination appends the lists to its arena (MSC_ERR_OOM when full).
 *   msc_hist_set_reset: a sparse set forgets every list (its arena is append-only otherwise): what a one-slot staging set does
 *                    between two queries. */
uint64_t msc_hist_packed_bytes(const msc_hist_set* set, uint64_t slot);
int      msc_hist_pack(msc_ctx* ctx, const msc_hist_set* set, const uint32_t* slots, uint64_t n, void* dev_dst, const uint64_t* offsets);
int      msc_hist_unpack(msc_ctx* ctx, msc_hist_set* set, const uint32_t* slots, uint64_t n, const void* dev_src, const uint64_t* offsets);
int      msc_hist_set_reset(msc_ctx* ctx, msc_hist_set* set);

/* get_mean / the mean of mean_shift_update (cluster/ClusterFactory.cpp:338-380,297-326) when the members of a list live on several
 * GPUs: SURVEY 8(e)'s reduction of partial column sums. n lists at once; list c = member_slots[offsets[c] .. offsets[c+1]) of THIS
 * rank's set (may be empty).
 *   msc_colsum_partial: the integer column sums of this rank's members. *dev_payload (library-owned, valid until the next call) is
 *     dense sets : uint64 [n][padded bins] followed by uint64 [n] member counts -> ALL-REDUCE (sum) it in place, payload_bytes / 8 words;
 *     sparse sets: a table {n, bytes, (members, offset) x n} and per list a packed sparse slot of the summed excesses -> ALL-GATHER
 *                  it, every rank padded to the largest payload_bytes.
 *   msc_colsum_nearest: dev_global = the reduced array (dense; world ignored) or the gathered payloads, bytes_per_rank apart (sparse).
 *     Every rank derives the same FP64 mean of each list (exact integer sums / total members: the single-GPU mean bit for bit),
 *     rounds it, and measures ITS members: nearest_pos[c] = position inside this rank's list c of its first member nearest the mean
 *     (DivergencePoint::distance_d, clutil/DivergencePoint.cpp:55-66), -1 for an empty list; nearest_dist[c] its distance;
 *     m_total_out[c] (nullable) = members of list c over all ranks. The caller folds the ranks' (distance, position) records.
 *   msc_colsum_list_bytes: device scratch one list costs (a driver sizes its chunks of centres by it).
 * msc_filter_batch: Trainer::filter (cluster/Trainer.cpp:123-141) of n centres against their lists in one pass -- the first stage of
 *   msc_update_centres alone; keep[i] = 1 iff pt_slots[i] survives the filter of its centre. */
uint64_t msc_colsum_list_bytes(const msc_hist_set* set);
int      msc_colsum_partial(msc_ctx* ctx, const msc_hist_set* set, const uint32_t* member_slots, const uint64_t* offsets, uint64_t n,
                            void** dev_payload, uint64_t* payload_bytes);
int      msc_colsum_nearest(msc_ctx* ctx, const msc_hist_set* set, const uint32_t* member_slots, const uint64_t* offsets, uint64_t n,
                            const void* dev_global, uint64_t bytes_per_rank, int world, int64_t* nearest_pos, double* nearest_dist,
                            uint64_t* m_total_out);
int      msc_filter_batch(msc_ctx* ctx, const msc_model* model, double cutoff, const msc_hist_set* centres, const uint32_t* centre_slots,
                          uint64_t n_centres, const msc_hist_set* pts, const uint32_t* pt_slots, const uint64_t* offsets, uint8_t* keep);

/* Plain device memory and the ctx's HIP stream for a caller that owns the communicator (rccl.h takes a hipStream_t: collectives
 * queued on this stream are ordered with the library's kernels without a host round trip). */
void*    msc_stream_handle(msc_ctx* ctx);
int      msc_device_malloc(msc_ctx* ctx, uint64_t bytes, void** out);
int      msc_device_free(msc_ctx* ctx, void* p);
int      msc_memcpy_to_host(msc_ctx* ctx, void* dst, const void* src_dev, uint64_t bytes);
int      msc_memcpy_to_device(msc_ctx* ctx, void* dst_dev, const void* src, uint64_t bytes);
int      msc_memcpy_device(msc_ctx* ctx, void* dst_dev, const void* src_dev, uint64_t bytes);      /* queued on the ctx stream, not waited for */
/* Page-locked host memory for result arrays that are filled call after call (the [n_q][m] outputs of msc_score_multi: into pageable
 * memory the runtime stages every copy through its own bounce buffers -- 0.6 ms of a 7 ms step for 6.4 MB of close flags). */
int      msc_host_alloc(msc_ctx* ctx, uint64_t bytes, void** out);
int      msc_host_free(msc_ctx* ctx, void* p);

#ifdef __cplusplus
}
#endif
#endif /* MESHCLUST2_HIP_H */
