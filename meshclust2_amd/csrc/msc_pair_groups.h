// msc_pair_groups.h -- host bookkeeping of msc_score_pair_list (msc_api_pairlist.hip): an explicit list of pairs (a_i, b_i) is grouped by its
// second slot with a stable sort, cut into chunks of a pair budget, each chunk described as segments (one second slot, a run of the
// permuted list), and a chunk's result rows are scattered back to the caller's order. Plain C++, no HIP types: the stand-alone check
// under tests/ builds this file alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

// One run of the permuted list that shares a second slot: permuted pairs [first, first + m). (Within a chunk `first` is relative to it.)
struct MscPairRun {
	uint32_t b_slot;
	uint64_t first;
	uint64_t m;
};

struct MscPairGroups {
	std::vector<uint64_t> perm;         // perm[j] = the caller's index of permuted pair j (stable: ascending inside a run)
	std::vector<MscPairRun> runs;       // ascending b_slot; the runs tile [0, n)
};

// b_slots == nullptr means slots 0 .. n-1 (every pair its own run, already in order)
static inline MscPairGroups msc_pair_group(const uint32_t* b_slots, uint64_t n) {
	MscPairGroups g;
	g.perm.resize((size_t)n);
	std::iota(g.perm.begin(), g.perm.end(), (uint64_t)0);
	auto b_of = [&](uint64_t i) -> uint32_t { return b_slots ? b_slots[i] : (uint32_t)i; };
	if (b_slots) std::stable_sort(g.perm.begin(), g.perm.end(), [&](uint64_t x, uint64_t y) { return b_slots[x] < b_slots[y]; });
	for (uint64_t j = 0; j < n; j++) {
		const uint32_t b = b_of(g.perm[(size_t)j]);
		if (g.runs.empty() || g.runs.back().b_slot != b) g.runs.push_back(MscPairRun{b, j, 0});
		g.runs.back().m++;
	}
	return g;
}

// The permuted list cut into chunks of at most max_pairs pairs (at least 1): chunk c = permuted pairs [cuts[c], cuts[c + 1]). A run longer
// than what is left of a chunk is cut as well -- the next chunk carries on with the same second slot.
static inline std::vector<uint64_t> msc_pair_chunks(uint64_t n, uint64_t max_pairs) {
	if (max_pairs < 1) max_pairs = 1;
	std::vector<uint64_t> cuts(1, 0);
	while (cuts.back() < n) cuts.push_back(cuts.back() + std::min<uint64_t>(max_pairs, n - cuts.back()));
	return cuts;
}

// The runs of chunk [p0, p1), `first` relative to p0, and for every pair of the chunk the index of its run; *max_m = its longest run.
static inline void msc_pair_chunk_runs(const MscPairGroups& g, uint64_t p0, uint64_t p1, std::vector<MscPairRun>& runs_out, std::vector<uint32_t>& pair_run_out,
                                       uint64_t* max_m) {
	runs_out.clear();
	pair_run_out.assign((size_t)(p1 - p0), 0u);
	uint64_t mm = 0;
	// first run that reaches past p0
	size_t r = (size_t)(std::upper_bound(g.runs.begin(), g.runs.end(), p0, [](uint64_t p, const MscPairRun& run) { return p < run.first + run.m; }) - g.runs.begin());
	for (; r < g.runs.size() && g.runs[r].first < p1; r++) {
		const uint64_t lo = std::max(g.runs[r].first, p0), hi = std::min(g.runs[r].first + g.runs[r].m, p1);
		for (uint64_t j = lo; j < hi; j++) pair_run_out[(size_t)(j - p0)] = (uint32_t)runs_out.size();
		runs_out.push_back(MscPairRun{g.runs[r].b_slot, lo - p0, hi - lo});
		mm = std::max(mm, hi - lo);
	}
	if (max_m) *max_m = mm;
}

// the first slots of chunk [p0, p1) in permuted order (a_slots == nullptr means slots 0 .. n-1)
static inline void msc_pair_chunk_a(const MscPairGroups& g, const uint32_t* a_slots, uint64_t p0, uint64_t p1, std::vector<uint32_t>& out) {
	out.resize((size_t)(p1 - p0));
	for (uint64_t j = p0; j < p1; j++) out[(size_t)(j - p0)] = a_slots ? a_slots[g.perm[(size_t)j]] : (uint32_t)g.perm[(size_t)j];
}

// rows [0, p1 - p0) of `src` (the chunk's results, `width` elements each) to their places in the caller's order
template <typename T>
static inline void msc_pair_scatter(const MscPairGroups& g, uint64_t p0, uint64_t p1, size_t width, const T* src, T* dst) {
	for (uint64_t j = p0; j < p1; j++) memcpy(dst + (size_t)g.perm[(size_t)j] * width, src + (size_t)(j - p0) * width, width * sizeof(T));
}
