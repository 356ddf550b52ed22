// query_groups_check.cpp -- stand-alone check of msc_query_groups (meshclust2_amd/csrc/msc_multi_plan.h; built and run by tests/test_query_groups_cpu.py with
// -fsanitize=address,undefined): which blocks of a call's plan share one build of the queries' side, how many under the cap and the arena's budget, and where
// each block's images and lists lie in the arena. Exit status 0 = every case held; a failed check prints its case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../meshclust2_amd/csrc/msc_multi_plan.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                              \
	do {                                                              \
		if (!(cond)) {                                                \
			fprintf(stderr, "FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond); \
			fprintf(stderr, __VA_ARGS__);                             \
			fprintf(stderr, "\n");                                    \
			g_failed++;                                               \
		}                                                             \
	} while (0)

typedef unsigned long long ull;
static const uint64_t kMiB = 1ull << 20, kBudget = 512 * kMiB, kBins9 = 262144;

// the rules, written out a second time over the result: returns the sizes of the groups in order
static std::vector<size_t> held(const char* what, const std::vector<MscGroupBlock>& blocks, uint64_t nbins, uint32_t cap, uint64_t budget) {
	std::vector<MscQueryGroup> groups(2);          // (the function clears what it is handed)
	groups[0].n = 99;
	msc_query_groups(blocks, nbins, cap, budget, groups);
	std::vector<int> seen(blocks.size(), 0);
	std::vector<size_t> sizes;
	size_t at = 0;
	for (const MscQueryGroup& g : groups) {
		sizes.push_back(g.n);
		CHECK(g.n >= 1 && g.first >= at && g.first + g.n <= blocks.size(), "%s: group [%zu, +%zu) after %zu of %zu", what, g.first, g.n, at, blocks.size());
		if (g.n < 1 || g.first + g.n > blocks.size()) return sizes;
		for (size_t i = at; i < g.first; i++) CHECK(!blocks[i].joins, "%s: block %zu joins and is in no group", what, i);
		at = g.first + g.n;
		CHECK(g.n <= (cap < 2 ? 1u : cap), "%s: %zu blocks under cap %u", what, g.n, cap);
		uint64_t longest = 0;
		for (size_t i = g.first; i < at; i++) {
			CHECK(blocks[i].joins && blocks[i].fold == g.fold, "%s: block %zu in a group of fold %u", what, i, g.fold);
			longest = std::max(longest, blocks[i].n_hot);
			seen[i]++;
		}
		// the strides hold every block's images and lists
		const uint64_t nbins_f = g.fold ? nbins / g.fold : nbins;
		CHECK(g.qt_stride == nbins * 32 && g.anib_stride == nbins_f * 64, "%s: image strides %llu %llu", what, (ull)g.qt_stride, (ull)g.anib_stride);
		CHECK(g.hot_stride >= longest && g.hot_stride < longest + 2 && (longest || !g.hot_stride), "%s: hot stride %llu, longest list %llu", what, (ull)g.hot_stride, (ull)longest);
		CHECK(g.hot_stride ? g.idx_stride >= nbins_f / 128 + 1 && g.idx_stride < nbins_f / 128 + 5 : g.idx_stride == 0, "%s: idx stride %llu", what, (ull)g.idx_stride);
		// regions in order, none overlapping, everything on 16 bytes
		const uint64_t off[7] = {g.qt_off, g.anib_off, g.hot_off, g.ptr_off, g.cursor_off, g.cnt_off, g.bytes};
		const uint64_t stride[6] = {g.qt_stride, g.anib_stride, g.hot_stride * 8, g.idx_stride * 4, g.idx_stride * 4, g.idx_stride * 4};
		CHECK(off[0] == 0, "%s: the arena starts at %llu", what, (ull)off[0]);
		for (int r = 0; r < 6; r++) {
			CHECK(off[r] % 16 == 0 && stride[r] % 16 == 0, "%s: region %d at %llu, stride %llu", what, r, (ull)off[r], (ull)stride[r]);
			CHECK(off[r] + g.n * stride[r] <= off[r + 1], "%s: region %d [%llu, +%zu x %llu) runs into %llu", what, r, (ull)off[r], g.n, (ull)stride[r], (ull)off[r + 1]);
		}
		CHECK(g.bytes == g.n * msc_group_block_bytes(nbins, g.fold, g.hot_stride), "%s: %llu bytes for %zu blocks", what, (ull)g.bytes, g.n);
		CHECK(g.n == 1 || g.bytes <= budget, "%s: %llu bytes over the budget %llu", what, (ull)g.bytes, (ull)budget);
		// why the group ends where it does: the run ends, the cap, or the budget (taken with the longest list of the run up to the cap)
		const bool run_ends = at == blocks.size() || !blocks[at].joins || blocks[at].fold != g.fold;
		if (!run_ends && g.n < (cap < 2 ? 1u : cap)) {
			size_t end = g.first;
			uint64_t run_longest = 0;
			while (end < blocks.size() && end - g.first < cap && blocks[end].joins && blocks[end].fold == g.fold) run_longest = std::max(run_longest, blocks[end++].n_hot);
			CHECK((g.n + 1) * msc_group_block_bytes(nbins, g.fold, (run_longest + 1) / 2 * 2) > budget, "%s: group [%zu, +%zu) could have taken one more", what, g.first, g.n);
		}
	}
	for (size_t i = at; i < blocks.size(); i++) CHECK(!blocks[i].joins, "%s: block %zu joins and is in no group", what, i);
	for (size_t i = 0; i < blocks.size(); i++) CHECK(seen[i] == (blocks[i].joins ? 1 : 0), "%s: block %zu in %d groups", what, i, seen[i]);
	return sizes;
}

static bool is(const std::vector<size_t>& got, std::initializer_list<size_t> want) { return got == std::vector<size_t>(want); }

int main() {
	const MscGroupBlock folded{true, 16, 0}, plain{true, 0, 0}, off{false, 0, 0};
	// the bytes of a block at k = 9: 8 MiB of planes + 1 MiB of folded tiles, or + 16 MiB of true ones
	CHECK(msc_group_block_bytes(kBins9, 16, 0) == 9 * kMiB && msc_group_block_bytes(kBins9, 0, 0) == 24 * kMiB, "bytes of a block at k = 9");
	// cap 0, 1, 2, 32 over 64 folded blocks (the benchmark's call): singles, pairs, two groups of 32 of 288 MiB
	CHECK(is(held("cap 0", std::vector<MscGroupBlock>(5, folded), kBins9, 0, kBudget), {1, 1, 1, 1, 1}), "cap 0");
	CHECK(is(held("cap 1", std::vector<MscGroupBlock>(5, folded), kBins9, 1, kBudget), {1, 1, 1, 1, 1}), "cap 1");
	CHECK(is(held("cap 2", std::vector<MscGroupBlock>(5, folded), kBins9, 2, kBudget), {2, 2, 1}), "cap 2");
	CHECK(is(held("cap 32", std::vector<MscGroupBlock>(64, folded), kBins9, 32, kBudget), {32, 32}), "cap 32");
	CHECK(is(held("cap 32, 70 blocks", std::vector<MscGroupBlock>(70, folded), kBins9, 32, kBudget), {32, 32, 6}), "cap 32, 70 blocks");
	{
		std::vector<MscQueryGroup> g;
		msc_query_groups(std::vector<MscGroupBlock>(64, folded), kBins9, 32, kBudget, g);
		CHECK(g.size() == 2 && g[0].bytes == 288 * kMiB, "a folded group of 32 at k = 9 takes 288 MiB");
	}
	// the budget: unfolded blocks of 24 MiB -- 21 fit 512 MiB; a budget of 48 MiB admits two, of 47 or of 24 one, of 1 byte still one
	CHECK(is(held("budget for 21", std::vector<MscGroupBlock>(50, plain), kBins9, 32, kBudget), {21, 21, 8}), "budget for 21");
	CHECK(is(held("budget for 2", std::vector<MscGroupBlock>(5, plain), kBins9, 32, 48 * kMiB), {2, 2, 1}), "budget for 2");
	CHECK(is(held("budget for 1", std::vector<MscGroupBlock>(3, plain), kBins9, 32, 47 * kMiB), {1, 1, 1}), "budget for 1");
	CHECK(is(held("budget of a block", std::vector<MscGroupBlock>(3, plain), kBins9, 32, 24 * kMiB), {1, 1, 1}), "budget of a block");
	CHECK(is(held("budget of a byte", std::vector<MscGroupBlock>(3, plain), kBins9, 32, 1), {1, 1, 1}), "budget of a byte");
	// a declined block, a short block, a second run (none of them joins) in the middle of a call; a change of fold cuts a group too
	{
		std::vector<MscGroupBlock> b(9, folded);
		b[2] = off;
		CHECK(is(held("a declined block", b, kBins9, 32, kBudget), {2, 6}), "a declined block");
		CHECK(is(held("a declined block, cap 2", b, kBins9, 2, kBudget), {2, 2, 2, 2}), "a declined block, cap 2");
		b[2] = folded; b[8] = off;
		CHECK(is(held("a short last block", b, kBins9, 32, kBudget), {8}), "a short last block");
		b[0] = off; b[4] = off;
		CHECK(is(held("blocks out at both ends and in the middle", b, kBins9, 32, kBudget), {3, 3}), "blocks out at both ends and in the middle");
		b[6] = plain;
		CHECK(is(held("one block unfolded", b, kBins9, 32, kBudget), {3, 1, 1, 1}), "one block unfolded");
	}
	// zero matrix blocks, and no blocks at all
	CHECK(held("nothing joins", std::vector<MscGroupBlock>(7, off), kBins9, 32, kBudget).empty(), "nothing joins");
	CHECK(held("no blocks", std::vector<MscGroupBlock>(), kBins9, 32, kBudget).empty(), "no blocks");
	// hot lists: one stride, the group's longest list (rounded to 16 bytes); the lists count against the budget; k = 8, k = 5 and other folds keep the alignment
	for (uint64_t nbins : {(uint64_t)1024, (uint64_t)65536, kBins9})
		for (uint32_t fold : {0u, 8u, 16u, 32u}) {
			if (fold && nbins / fold < 256) continue;
			std::vector<MscGroupBlock> b;
			for (uint64_t i = 0; i < 40; i++) b.push_back(MscGroupBlock{i % 11 != 7, fold, i % 5 == 0 ? 0 : (i * 2654435761ull) % 777});
			char what[64];
			snprintf(what, sizeof what, "lists, %llu bins, fold %u", (ull)nbins, fold);
			for (uint32_t cap : {2u, 3u, 32u}) held(what, b, nbins, cap, kBudget);
			held(what, b, nbins, 32, 5 * msc_group_block_bytes(nbins, fold, 300));
		}
	{
		std::vector<MscGroupBlock> b(4, folded);
		b[1].n_hot = 5; b[3].n_hot = 131072;
		std::vector<MscQueryGroup> g;
		msc_query_groups(b, kBins9, 2, kBudget, g);
		CHECK(g.size() == 2 && g[0].hot_stride == 6 && g[1].hot_stride == 131072 && g[0].idx_stride == 132 && g[1].idx_stride == 132, "strides of the hot lists");
		held("a long list", b, kBins9, 2, kBudget);
	}
	if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
	printf("query groups ok\n");
	return 0;
}
