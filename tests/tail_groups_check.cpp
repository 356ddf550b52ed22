// tail_groups_check.cpp -- stand-alone check of msc_tail_groups (meshclust2_amd/csrc/msc_multi_plan.h; built and run by tests/test_tail_groups_cpu.py with
// -fsanitize=address,undefined): which folded blocks of a call's plan share one tail, how many under the cap, the side's budget and the 32-bit pair count,
// how the call's final groups halve down to one block, and where each block's arrays lie in the side. Exit status 0 = every case held; a failed check
// prints its case and exits 1.
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
static const uint64_t kGiB = 1ull << 30, kM = 100000;

// the blocks of a call: n of them, in query groups of qg, all joining
static std::vector<MscTailBlock> call(size_t n, size_t qg, uint64_t n_hot = 7) {
	std::vector<MscTailBlock> b;
	for (size_t i = 0; i < n; i++) b.push_back(MscTailBlock{true, (int)(i / qg), n_hot});
	return b;
}

// the ramp, a second time: the most blocks a group that starts with `left` blocks of the call remaining may take
static uint64_t ramp_limit(uint64_t left, uint32_t cap) {
	uint64_t points[40], n = 0;
	for (uint64_t p = cap; p; p /= 2) points[n++] = p;
	points[n++] = 0;
	for (uint64_t i = 0; i < n; i++) if (points[i] < left) return left - points[i];
	return 1;
}

// the rules, written out a second time over the result: returns the sizes of the groups in order
static std::vector<size_t> held(const char* what, const std::vector<MscTailBlock>& blocks, uint64_t m, uint32_t slices, uint32_t cap, uint64_t budget, bool ramp) {
	std::vector<MscTailGroup> groups(2);          // (the function clears what it is handed)
	groups[0].n = 99;
	msc_tail_groups(blocks, m, slices, cap, budget, ramp, groups);
	std::vector<int> seen(blocks.size(), 0);
	std::vector<size_t> sizes;
	size_t at = 0;
	auto joins = [&](size_t i) { return blocks[i].joins && blocks[i].qgroup >= 0; };
	for (const MscTailGroup& g : groups) {
		sizes.push_back(g.n);
		CHECK(g.n >= 1 && g.first >= at && g.first + g.n <= blocks.size(), "%s: group [%zu, +%zu) after %zu of %zu", what, g.first, g.n, at, blocks.size());
		if (g.n < 1 || g.first + g.n > blocks.size()) return sizes;
		for (size_t i = at; i < g.first; i++) CHECK(!joins(i), "%s: block %zu joins and is in no group", what, i);
		at = g.first + g.n;
		const uint64_t limit = cap < 2 ? 1 : cap;
		CHECK(g.n <= limit, "%s: %zu blocks under cap %u", what, g.n, cap);
		bool any_hot = false;
		for (size_t i = g.first; i < at; i++) {
			CHECK(joins(i) && blocks[i].qgroup == blocks[g.first].qgroup, "%s: block %zu (query group %d) in a group of query group %d", what, i, blocks[i].qgroup, blocks[g.first].qgroup);
			any_hot = any_hot || blocks[i].n_hot;
			seen[i]++;
		}
		// the pairs of one launch fit 32 bits
		CHECK(g.n == 1 || msc_list_pairs_fit((uint64_t)g.n * 128 * m), "%s: %zu blocks x 128 x %llu pairs", what, g.n, (ull)m);
		// the strides hold every block's arrays
		const uint64_t cap_entries = 128 * m / 64;
		CHECK(g.list_cap == cap_entries && g.list_stride >= cap_entries && g.list_stride < cap_entries + 4, "%s: list capacity %u, stride %llu", what, g.list_cap, (ull)g.list_stride);
		CHECK(g.min_stride == (uint64_t)slices * m * 128 * 4 && g.flags_stride == 128 * m && g.words_stride >= 2, "%s: strides %llu %llu %llu", what, (ull)g.min_stride, (ull)g.flags_stride,
		      (ull)g.words_stride);
		CHECK(g.diff_stride == (any_hot ? m * 128 * 4 : 0), "%s: P2 stride %llu", what, (ull)g.diff_stride);
		// regions in order, none overlapping, everything on 16 bytes
		const uint64_t off[7] = {g.min_off, g.diff_off, g.flags_off, g.list_off, g.emd_off, g.words_off, g.bytes};
		const uint64_t stride[6] = {g.min_stride, g.diff_stride, g.flags_stride, g.list_stride * 4, g.list_stride * 8, g.words_stride * 4};
		CHECK(off[0] == 0, "%s: the side starts at %llu", what, (ull)off[0]);
		for (int r = 0; r < 6; r++) {
			CHECK(off[r] % 16 == 0 && stride[r] % 16 == 0, "%s: region %d at %llu, stride %llu", what, r, (ull)off[r], (ull)stride[r]);
			CHECK(off[r] + g.n * stride[r] <= off[r + 1], "%s: region %d [%llu, +%zu x %llu) runs into %llu", what, r, (ull)off[r], g.n, (ull)stride[r], (ull)off[r + 1]);
		}
		CHECK(g.bytes == g.n * msc_tail_block_bytes(m, slices, any_hot), "%s: %llu bytes for %zu blocks", what, (ull)g.bytes, g.n);
		CHECK(g.n == 1 || g.bytes <= budget, "%s: %llu bytes over the budget %llu", what, (ull)g.bytes, (ull)budget);
		// the ramp: no group crosses a point where cap, cap/2, ..., 1 blocks of the call remain
		const uint64_t ramp_most = ramp && cap >= 2 ? ramp_limit(blocks.size() - g.first, cap) : limit;
		CHECK(g.n <= ramp_most, "%s: group [%zu, +%zu) crosses the ramp (%llu at most)", what, g.first, g.n, (ull)ramp_most);
		// why the group ends where it does: the run ends, the cap, the ramp, the pair count, or the budget (with P2 if any block of the run up to the limit has a list)
		const bool run_ends = at == blocks.size() || !joins(at) || blocks[at].qgroup != blocks[g.first].qgroup;
		if (!run_ends && g.n < std::min(limit, ramp_most) && msc_list_pairs_fit((uint64_t)(g.n + 1) * 128 * m)) {
			bool run_hot = false;
			for (size_t i = g.first; i < blocks.size() && i - g.first < std::min(limit, ramp_most) && joins(i) && blocks[i].qgroup == blocks[g.first].qgroup; i++) run_hot = run_hot || blocks[i].n_hot;
			CHECK((g.n + 1) * msc_tail_block_bytes(m, slices, run_hot) > budget, "%s: group [%zu, +%zu) could have taken one more", what, g.first, g.n);
		}
	}
	for (size_t i = at; i < blocks.size(); i++) CHECK(!joins(i), "%s: block %zu joins and is in no group", what, i);
	for (size_t i = 0; i < blocks.size(); i++) CHECK(seen[i] == (joins(i) ? 1 : 0), "%s: block %zu in %d groups", what, i, seen[i]);
	return sizes;
}

static bool is(const std::vector<size_t>& got, std::initializer_list<size_t> want) { return got == std::vector<size_t>(want); }
static bool ends_with(const std::vector<size_t>& got, std::initializer_list<size_t> want) {
	const std::vector<size_t> w(want);
	return got.size() >= w.size() && std::equal(w.begin(), w.end(), got.end() - w.size());
}

int main() {
	// the bytes of a block of the benchmark's call (100 000 candidates, one slice, a hot list): P1 and P2 of 51.2 MB, 12.8 MB of flags, 2.4 MB of lists
	CHECK(msc_tail_block_bytes(kM, 1, true) == 2 * 51200000ull + 12800000ull + 200000ull * 12 + 16, "bytes of a block of the benchmark's call");
	CHECK(8 * msc_tail_block_bytes(kM, 1, true) <= kGiB && 10 * msc_tail_block_bytes(kM, 1, true) > kGiB, "eight such blocks fit 1 GiB, ten do not");
	// every count of blocks, cap and size of the query groups, with the ramp and without: the rules hold
	for (size_t n : {0, 1, 2, 5, 8, 9, 64, 65})
		for (uint32_t cap : {0u, 1u, 2u, 8u})
			for (size_t qg : {2, 8, 32})
				for (bool ramp : {false, true}) {
					char what[96];
					snprintf(what, sizeof what, "%zu blocks, cap %u, query groups of %zu, ramp %d", n, cap, qg, (int)ramp);
					const std::vector<size_t> got = held(what, call(n, qg), kM, 1, cap, kGiB, ramp);
					size_t sum = 0;
					for (size_t s : got) sum += s;
					CHECK(sum == n, "%s: %zu blocks in groups", what, sum);
					if (cap < 2) CHECK(got == std::vector<size_t>(n, 1), "%s: singles", what);
				}
	// the benchmark's call: 64 blocks in two query groups of 32
	CHECK(is(held("64, no ramp", call(64, 32), kM, 1, 8, kGiB, false), {8, 8, 8, 8, 8, 8, 8, 8}), "64 blocks, no ramp");
	CHECK(is(held("64, ramp", call(64, 32), kM, 1, 8, kGiB, true), {8, 8, 8, 8, 8, 8, 8, 4, 2, 1, 1}), "64 blocks, ramp");
	CHECK(is(held("8, ramp", call(8, 32), kM, 1, 8, kGiB, true), {4, 2, 1, 1}), "8 blocks, ramp: 4, 2, 1, 1");
	CHECK(is(held("65, ramp", call(65, 32), kM, 1, 8, kGiB, true), {8, 8, 8, 8, 8, 8, 8, 1, 4, 2, 1, 1}), "65 blocks, ramp");
	CHECK(is(held("65, no ramp", call(65, 32), kM, 1, 8, kGiB, false), {8, 8, 8, 8, 8, 8, 8, 8, 1}), "65 blocks, no ramp");
	CHECK(is(held("9, ramp", call(9, 32), kM, 1, 8, kGiB, true), {1, 4, 2, 1, 1}), "9 blocks, ramp");
	CHECK(is(held("5, ramp", call(5, 32), kM, 1, 8, kGiB, true), {1, 2, 1, 1}), "5 blocks, ramp");
	CHECK(is(held("5, cap 2, ramp", call(5, 32), kM, 1, 2, kGiB, true), {2, 1, 1, 1}), "5 blocks, cap 2, ramp");
	CHECK(is(held("5, cap 2", call(5, 32), kM, 1, 2, kGiB, false), {2, 2, 1}), "5 blocks, cap 2");
	// the ramp's final groups are ..., 2, 1 and the block left over, whatever comes before
	for (size_t n : {8, 9, 64, 65}) CHECK(ends_with(held("ramp's end", call(n, 32), kM, 1, 8, kGiB, true), {4, 2, 1, 1}), "the ramp's end, %zu blocks", n);
	// tail groups stop at the query groups' ends
	CHECK(is(held("query groups of 2", call(8, 2), kM, 1, 8, kGiB, false), {2, 2, 2, 2}), "query groups of 2");
	CHECK(is(held("query groups of 2, ramp", call(8, 2), kM, 1, 8, kGiB, true), {2, 2, 2, 1, 1}), "query groups of 2, ramp");
	CHECK(is(held("query groups of 8, 20 blocks", call(20, 8), kM, 1, 8, kGiB, false), {8, 8, 4}), "query groups of 8");
	CHECK(is(held("query groups of 32, cap 8, 40 blocks", call(40, 32), kM, 1, 8, kGiB, false), {8, 8, 8, 8, 8}), "query groups of 32");
	CHECK(is(held("query groups of 3, cap 2", call(7, 3), kM, 1, 2, kGiB, false), {2, 1, 2, 1, 1}), "query groups of 3, cap 2");
	// a block that does not join in the middle (a declined block, a second run, another tail), and one in no query group
	{
		std::vector<MscTailBlock> b = call(9, 32);
		b[3].joins = false;
		CHECK(is(held("a block out", b, kM, 1, 8, kGiB, false), {3, 5}), "a block out in the middle");
		CHECK(is(held("a block out, ramp", b, kM, 1, 8, kGiB, true), {1, 2, 1, 2, 1, 1}), "a block out in the middle, ramp");
		b[3].joins = true; b[3].qgroup = -1;
		CHECK(is(held("a block in no query group", b, kM, 1, 8, kGiB, false), {3, 5}), "a block in no query group");
		b[8].joins = false;
		CHECK(is(held("a short last block", b, kM, 1, 8, kGiB, false), {3, 4}), "a short last block");
	}
	CHECK(held("nothing joins", std::vector<MscTailBlock>(7, MscTailBlock{false, 0, 0}), kM, 1, 8, kGiB, true).empty(), "nothing joins");
	// a budget that holds three blocks; of a block, of a byte: singles
	{
		const uint64_t one = msc_tail_block_bytes(kM, 1, true);
		CHECK(is(held("budget for 3", call(8, 32), kM, 1, 8, 3 * one, false), {3, 3, 2}), "a budget for three blocks");
		CHECK(is(held("budget for 3 less a byte", call(8, 32), kM, 1, 8, 3 * one - 1, false), {2, 2, 2, 2}), "a budget a byte short of three blocks");
		CHECK(is(held("budget for 3, ramp", call(16, 32), kM, 1, 8, 3 * one, true), {3, 3, 2, 3, 1, 2, 1, 1}), "a budget for three blocks, ramp");
		CHECK(is(held("budget of a block", call(3, 32), kM, 1, 8, one, false), {1, 1, 1}), "a budget of one block");
		CHECK(is(held("budget of a byte", call(3, 32), kM, 1, 8, 1, false), {1, 1, 1}), "a budget of a byte");
		// no hot list in any block: no P2, and more blocks fit the same budget
		CHECK(is(held("no lists", call(8, 32, 0), kM, 1, 8, 3 * one, false), {5, 3}), "no hot lists: five blocks where three fitted");
		std::vector<MscTailBlock> b = call(8, 32, 0);
		b[6].n_hot = 1;
		held("one list in the run", b, kM, 1, 8, 3 * one, false);
	}
	// the pair count of one launch: n x 128 x m at 2^32 - 1 and at 2^32
	{
		const uint64_t m_fit = 0xffffffffull / (128 * 4), m_over = (1ull << 32) / (128 * 4);          // four blocks: 4 x 128 x m = 2^32 - 512 (the most under 2^32 - 1), and 2^32
		CHECK(4 * 128 * m_fit <= 0xffffffffull && 4 * 128 * (m_fit + 1) > 0xffffffffull && 4 * 128 * m_over == (1ull << 32), "the two candidate counts");
		CHECK(is(held("pairs fit", call(8, 32, 0), m_fit, 1, 4, ~0ull, false), {4, 4}), "four blocks of pairs under 2^32");
		CHECK(is(held("pairs over", call(8, 32, 0), m_over, 1, 4, ~0ull, false), {3, 3, 2}), "four blocks of 2^32 pairs: three");
		CHECK(msc_list_pairs_fit(0xffffffffull) && !msc_list_pairs_fit(1ull << 32), "msc_list_pairs_fit at 2^32 - 1 and 2^32");
		CHECK(is(held("one block of all pairs", call(3, 32, 0), 0xffffffffull / 128, 1, 8, ~0ull, false), {1, 1, 1}), "a block of 2^32 - 128 pairs stays alone");
	}
	// other candidate counts, slices: alignment holds (m odd: the list stride is rounded up)
	for (uint64_t m : {(uint64_t)1, (uint64_t)3, (uint64_t)601, (uint64_t)640, (uint64_t)99999})
		for (uint32_t slices : {1u, 2u, 8u})
			for (uint32_t cap : {2u, 3u, 8u}) {
				char what[64];
				snprintf(what, sizeof what, "m %llu, %u slices, cap %u", (ull)m, slices, cap);
				std::vector<MscTailBlock> b;
				for (size_t i = 0; i < 40; i++) b.push_back(MscTailBlock{i % 11 != 7, (int)(i / 6) - (i % 13 == 5 ? 100 : 0), i % 3 ? i : 0});
				held(what, b, m, slices, cap, kGiB, false);
				held(what, b, m, slices, cap, kGiB, true);
				held(what, b, m, slices, cap, 4 * msc_tail_block_bytes(m, slices, true), true);
			}
	if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
	printf("tail groups ok\n");
	return 0;
}
