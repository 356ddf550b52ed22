// msc_multi_plan.h -- the host arithmetic of the Q x M calls (msc_api_multi.hip, msc_api_pairs.hip): how msc_score_multi cuts its queries
// into blocks, how a block's candidates are cut into chunks, and what a block on the matrix cores decides about its stages. Free of HIP, so that tests/multi_plan_check.cpp builds it with g++ alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct MscMultiBlock {
	uint64_t q0, nq;          // queries [q0, q0 + nq) of the call
	bool matrix;              // the block runs on the matrix cores
};

// The blocks of one msc_score_multi call. With kb_fit (the matrix cores can take the call) blocks are of 128 consecutive queries, the last
// one short; otherwise of 64. A block of two queries or more is offered to the matrix cores: declines(q0, nq) says whether it stays off them
// (its hot list is too long, or no ranks mirror stands while the earth mover's distance is wanted). A declined block of more than 64 becomes
// consecutive sub-blocks of 64 for the older routes. A trailing block of one query is kept (it takes the per-query route).
template <class Declines>
inline void msc_multi_plan(uint64_t n_q, bool kb_fit, Declines declines, std::vector<MscMultiBlock>& out) {
	out.clear();
	const uint64_t blk = kb_fit ? 128 : 64;
	for (uint64_t q0 = 0; q0 < n_q; q0 += blk) {
		const uint64_t nq = std::min(blk, n_q - q0);
		const bool matrix = kb_fit && nq >= 2 && !declines(q0, nq);
		for (uint64_t s = 0; s < nq; s += matrix ? nq : 64) out.push_back(MscMultiBlock{q0 + s, matrix ? nq : std::min<uint64_t>(64, nq - s), matrix});
	}
}

// The candidate chunks of a block: m candidates, of which `cap` fit one launch's scratch (never taken below 256), in n equal chunks.
struct MscCandChunks { uint64_t chunk, n; };
inline MscCandChunks msc_cand_chunks(uint64_t m, uint64_t cap) {
	const uint64_t c0 = std::min(std::max<uint64_t>(cap, 256), m);
	const uint64_t n = (m + c0 - 1) / c0;
	return MscCandChunks{(m + n - 1) / n, n};
}

// ---- a block on the matrix cores (run_matrix, msc_api_multi.hip): the plain facts its stage decisions rest on, the decisions, and one
// function between them. The facts are filled where the block begins (matrix_facts), the two environment switches among them.
struct MscMatrixFacts {
	bool model = false, screen_ok = false;                        // a model is given; its statistics admit the f32 screen (MscDevModel::screen_ok)
	bool close = false, sum = false, csum = false, raw = false;   // what the caller wants of the block
	bool want_div = false, want_grp = false;                      // a divergence / group statistic is wanted ...
	bool div_pass = false;                                        // ... and the divergence sums come from a merge pass per query (not from cells)
	bool no_screen = false, no_prep = false;                      // MSC_NO_SCREEN, MSC_GEMM_NO_PREP
	bool queued = false, emd_ranks = false;                       // the route: queued behind the block before; the distance from the ranks mirrors
	bool block_pipe = false, emd_bounds = false;                  // the context: msc_set_block_pipe, msc_set_emd_bounds
	uint32_t fold_screen = 0;                                     // ... msc_set_fold_screen
	bool emd_decides = false, fold_overflows = false;             // the model is remembered for overflowing the list of open pairs / the folded stage's
	uint64_t rk_pitch_c = 0, rk_pitch_q = 0;                      // the ranks mirrors of the candidates' and the queries' set: pitch,
	bool moments_c = false, moments_q = false;                    // ... whether the two moments per slot stand beside it,
	bool kbf_c = false, kbf_q = false;                            // ... whether the set carries a folded mirror,
	uint32_t kbf_fold_c = 0, kbf_fold_q = 0;                      // ... and of which fold
	bool second_run = false;                                      // the block ran folded and its list overflowed: this is its second run, with the true product
	uint64_t n_q = 0, m = 0, chunk = 0;                           // queries of the block, candidates of the call, candidates per launch
};

struct MscMatrixStages {
	bool screen = false;             // only the close flags are wanted: decided in f32 with an error bound, FP64 for the pairs the bound leaves open
	bool walk_counted = false;       // ... with the distance from the ranks mirrors: the block counts in msc_last_emd_walk
	bool bounds_call = false;        // ... from bounds of the distance first (msc_emd_list.hip), in every chunk of 64 pairs and more
	uint32_t fold = 0;               // ... with the product over bits folded fold-to-1 (msc_fold.h); 0: the true product
	bool piped = false;              // the block's stages on the three streams of the pipe
	bool own_prep_stream = false;    // ... the queries' side on the prep stream
	bool counted = false;            // the block's counters are bumped (not in a second run: it was counted when it ran folded)
};

inline bool msc_list_pairs_fit(uint64_t pairs) { return pairs >= 64 && pairs <= 0xffffffffull; }          // (fewer than 64 pairs: a list of no entries; the list holds 32-bit pair indices)

inline MscMatrixStages msc_matrix_stages(const MscMatrixFacts& f) {
	MscMatrixStages s;
	s.screen = f.model && f.screen_ok && f.close && !f.sum && !f.csum && !f.raw && !f.want_div && !f.want_grp && !f.no_screen;
	s.walk_counted = s.screen && f.emd_ranks;
	s.bounds_call = s.walk_counted && f.emd_bounds && !f.emd_decides && f.rk_pitch_c == f.rk_pitch_q && f.moments_c && f.moments_q;
	const bool folds = s.bounds_call && !f.second_run && f.chunk == f.m && msc_list_pairs_fit(f.n_q * f.m) && !f.fold_overflows && f.kbf_c && f.kbf_q &&
	                   f.kbf_fold_c == f.fold_screen && f.kbf_fold_q == f.fold_screen;
	s.fold = folds ? f.fold_screen : 0;
	s.piped = f.queued && f.chunk == f.m && !f.div_pass && !f.want_grp && f.block_pipe;
	s.own_prep_stream = s.piped && !f.no_prep;
	s.counted = !f.second_run;
	return s;
}

// The tail of a chunk of mc candidates, one of three forms:
//   scored  the optional rank walk of every pair, then the epilogue
//   bounds  the list stage (bound screen, walk and FP64 evaluation of the listed pairs), then the dense walk and the epilogue predicated on the
//           list's overflow word, then the kernel that closes the list
//   folded  the list stage on the folded words (with the listed pairs' exact counts), then the closing kernel with the block's fold_over word
enum MscMatrixTail { MSC_TAIL_SCORED, MSC_TAIL_BOUNDS, MSC_TAIL_FOLDED };
struct MscMatrixChunk { bool bounds; uint32_t open_cap; MscMatrixTail tail; };
inline MscMatrixChunk msc_matrix_chunk(const MscMatrixStages& s, uint64_t n_q, uint64_t mc) {
	const bool bounds = s.bounds_call && msc_list_pairs_fit(n_q * mc);
	return MscMatrixChunk{bounds, bounds ? (uint32_t)(n_q * mc / 64) : 0, !bounds ? MSC_TAIL_SCORED : s.fold ? MSC_TAIL_FOLDED : MSC_TAIL_BOUNDS};
}

// ---- the queries' side of several blocks in one set of launches (msc_set_query_groups; group_side, msc_api_multi.hip). Consecutive blocks of
// a call form a GROUP when each of them `joins` (it takes the matrix cores piped, with 128 query rows, and is not a second run) and they agree
// on the fold. A group's images lie in one arena, region by region, block j of the group at a region's offset + j strides:
//   qT      the transposed planes of the TRUE bins                           nbins x 32 bytes a block
//   anib    the nibble tiles of the bins the product runs on                 nbins / fold x 64 bytes
//   hot     the hot lists, one stride for all: the group's longest list      8 bytes an entry
//   ptr, cursor, cnt   the lists' step arrays                                nbins / fold / 128 + 1 words each
// Size of a group: the blocks left of the run, at most `cap`, at most what `budget` bytes hold (never fewer than one: a group of one block is
// left to the per-block path, as is every block with cap < 2). Every offset and stride is a multiple of 16 bytes.
struct MscGroupBlock { bool joins; uint32_t fold; uint64_t n_hot; };
struct MscQueryGroup {
	size_t first = 0, n = 0;                 // blocks [first, first + n) of the plan
	uint32_t fold = 0;
	uint64_t hot_stride = 0, idx_stride = 0; // entries of a block's hot list; words of each of its three step arrays (0, 0: no block of the group has a list)
	uint64_t qt_stride = 0, anib_stride = 0; // bytes
	uint64_t qt_off = 0, anib_off = 0, hot_off = 0, ptr_off = 0, cursor_off = 0, cnt_off = 0, bytes = 0;          // byte offsets of the regions; the arena's size
};

inline uint64_t msc_group_block_bytes(uint64_t nbins, uint32_t fold, uint64_t hot_stride) {
	const uint64_t nbins_f = fold ? nbins / fold : nbins, idx = hot_stride ? (nbins_f / 128 + 1 + 3) / 4 * 4 : 0;
	return nbins * 32 + nbins_f * 64 + hot_stride * 8 + 3 * idx * sizeof(uint32_t);
}

inline void msc_query_groups(const std::vector<MscGroupBlock>& blocks, uint64_t nbins, uint32_t cap, uint64_t budget, std::vector<MscQueryGroup>& out) {
	out.clear();
	const size_t limit = std::max<uint32_t>(cap, 1);
	for (size_t i = 0; i < blocks.size();) {
		if (!blocks[i].joins) { i++; continue; }
		size_t end = i;
		while (end < blocks.size() && end - i < limit && blocks[end].joins && blocks[end].fold == blocks[i].fold) end++;
		auto longest = [&](size_t n) { uint64_t h = 0; for (size_t j = i; j < i + n; j++) h = std::max(h, blocks[j].n_hot); return (h + 1) / 2 * 2; };
		MscQueryGroup g;
		g.first = i; g.fold = blocks[i].fold;
		const uint64_t fit = budget / msc_group_block_bytes(nbins, g.fold, longest(end - i));          // (with the longest list of the whole run: a shorter group's is no longer)
		g.n = (size_t)std::min<uint64_t>(end - i, std::max<uint64_t>(fit, 1));
		const uint64_t nbins_f = g.fold ? nbins / g.fold : nbins;
		g.hot_stride = longest(g.n);
		g.idx_stride = g.hot_stride ? (nbins_f / 128 + 1 + 3) / 4 * 4 : 0;
		g.qt_stride = nbins * 32; g.anib_stride = nbins_f * 64;
		g.qt_off = 0;
		g.anib_off = g.qt_off + g.n * g.qt_stride;
		g.hot_off = g.anib_off + g.n * g.anib_stride;
		g.ptr_off = g.hot_off + g.n * g.hot_stride * 8;
		g.cursor_off = g.ptr_off + g.n * g.idx_stride * sizeof(uint32_t);
		g.cnt_off = g.cursor_off + g.n * g.idx_stride * sizeof(uint32_t);
		g.bytes = g.cnt_off + g.n * g.idx_stride * sizeof(uint32_t);
		out.push_back(g);
		i += g.n;
	}
}

// ---- the folded tail of several blocks in one set of launches (msc_set_tail_groups; group_tail, msc_api_multi.hip). The products stay one launch per
// block; what runs behind them -- bound screen, the listed pairs' exact counts, walk and FP64 evaluation, the closing kernel, the close counts, the
// flags' copy home -- runs once for a TAIL GROUP: a run of consecutive blocks that each `joins` (piped, 128 query rows, in a query group, not a second
// run, one chunk, the folded tail) and lie in ONE query group (their qT sit at one stride in its arena). A group's arrays lie in one buffer (two such
// sides take turns), region by region, block j at a region's offset + j strides:
//   min     P1 of the product, every slice                    slices x m x 128 int32
//   diff    P2 (only where a block of the group has a hot list)        m x 128 int32
//   flags   the close flags, query-major: the group's rows are contiguous, here and at the caller's        128 x m bytes
//   list, emd   the open pairs and their distances            128 m / 64 entries each (the stride rounded up to 4 entries)
//   words   {count, overflow} of a block's list               4 words a block (two used)
// Size of a group: at most `cap` blocks, at most what `budget` bytes hold, at most what keeps n x 128 x m pairs within msc_list_pairs_fit (never
// fewer than one block: a group of one is left to the per-block path, as is every block with cap < 2). Every offset and stride is a multiple of 16 bytes.
// ramp: a group's flags leave on the copy stream under the NEXT group's kernels, so the last group's copy is exposed. The call's final `cap` blocks
// are therefore cut cap/2, cap/4, ..., 1 and the one left over alone: no group crosses a point where cap, cap/2, cap/4, ..., 1 blocks of the call remain.
struct MscTailBlock { bool joins; int qgroup; uint64_t n_hot; };          // qgroup: the block's query group of the call (-1: none, and then it does not join)
struct MscTailGroup {
	size_t first = 0, n = 0;                 // blocks [first, first + n) of the plan
	uint32_t list_cap = 0;                   // entries a block's list holds: 128 m / 64
	uint64_t min_stride = 0, diff_stride = 0, flags_stride = 0;          // bytes (diff_stride 0: no block of the group has a hot list)
	uint64_t list_stride = 0, words_stride = 0;                          // entries of list and emd; words
	uint64_t min_off = 0, diff_off = 0, flags_off = 0, list_off = 0, emd_off = 0, words_off = 0, bytes = 0;          // byte offsets of the regions; the side's size
};

inline uint64_t msc_tail_list_stride(uint64_t m) { return (128 * m / 64 + 3) / 4 * 4; }
inline uint64_t msc_tail_block_bytes(uint64_t m, uint32_t slices, bool diff) {
	return (uint64_t)slices * m * 128 * sizeof(int32_t) + (diff ? m * 128 * sizeof(int32_t) : 0) + 128 * m + msc_tail_list_stride(m) * (sizeof(uint32_t) + sizeof(uint64_t)) + 4 * sizeof(uint32_t);
}

inline void msc_tail_groups(const std::vector<MscTailBlock>& blocks, uint64_t m, uint32_t slices, uint32_t cap, uint64_t budget, bool ramp, std::vector<MscTailGroup>& out) {
	out.clear();
	if (m == 0 || slices == 0) return;
	const size_t total = blocks.size();
	const uint64_t pairs_fit = 0xffffffffull / (128 * m);          // blocks whose pairs the 32-bit row arithmetic of one launch holds
	for (size_t i = 0; i < total;) {
		if (!blocks[i].joins || blocks[i].qgroup < 0) { i++; continue; }
		uint64_t limit = std::max<uint32_t>(cap, 1);
		if (ramp && cap >= 2) {          // the nearest of the points cap, cap/2, ..., 1, 0 (blocks that remain) ahead of this block
			const uint64_t left = total - i;
			uint64_t stop = cap;
			while (stop >= left) stop /= 2;
			limit = std::min<uint64_t>(limit, left - stop);
		}
		size_t end = i;
		while (end < total && end - i < limit && blocks[end].joins && blocks[end].qgroup == blocks[i].qgroup) end++;
		auto any_hot = [&](size_t n) { for (size_t j = i; j < i + n; j++) if (blocks[j].n_hot) return true; return false; };
		const uint64_t fit = budget / msc_tail_block_bytes(m, slices, any_hot(end - i));          // (with P2 if any block of the run has a hot list: a shorter group needs no more)
		MscTailGroup g;
		g.first = i;
		g.n = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(end - i, fit), pairs_fit));
		g.list_cap = (uint32_t)(128 * m / 64);
		g.min_stride = (uint64_t)slices * m * 128 * sizeof(int32_t);
		g.diff_stride = any_hot(g.n) ? m * 128 * sizeof(int32_t) : 0;
		g.flags_stride = 128 * m;
		g.list_stride = msc_tail_list_stride(m); g.words_stride = 4;
		g.min_off = 0;
		g.diff_off = g.min_off + g.n * g.min_stride;
		g.flags_off = g.diff_off + g.n * g.diff_stride;
		g.list_off = g.flags_off + g.n * g.flags_stride;
		g.emd_off = g.list_off + g.n * g.list_stride * sizeof(uint32_t);
		g.words_off = g.emd_off + g.n * g.list_stride * sizeof(uint64_t);
		g.bytes = g.words_off + g.n * g.words_stride * sizeof(uint32_t);
		out.push_back(g);
		i += g.n;
	}
}
