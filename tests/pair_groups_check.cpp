// pair_groups_check.cpp -- stand-alone check of meshclust2_amd/csrc/msc_pair_groups.h (built and run by tests/test_abi_pair_list_cpu.py with
// -fsanitize=address,undefined): grouping by second slot, chunking by a pair budget, the segments of a chunk and the scatter back to the
// caller's order, each against a brute-force map. Exit status 0 = every case held; a failed check prints its case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../meshclust2_amd/csrc/msc_pair_groups.h"

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

// value a pair "scores": a function of its two slots and of nothing else
static uint64_t score_of(uint32_t a, uint32_t b) { return (uint64_t)a * 1000003ull + (uint64_t)b * 7919ull + 1; }

static void run_case(const char* name, const std::vector<uint32_t>& a, const std::vector<uint32_t>* b_in, uint64_t budget) {
	const uint64_t n = a.size();
	const uint32_t* b = b_in ? b_in->data() : nullptr;
	auto b_of = [&](uint64_t i) -> uint32_t { return b ? b[i] : (uint32_t)i; };
	const MscPairGroups g = msc_pair_group(b, n);
	// perm is a permutation, runs tile [0, n) in ascending distinct b, stable inside a run
	CHECK(g.perm.size() == n, "%s", name);
	std::vector<int> seen((size_t)n, 0);
	for (uint64_t j = 0; j < n; j++) { CHECK(g.perm[j] < n, "%s j=%llu", name, (unsigned long long)j); if (g.perm[j] < n) seen[(size_t)g.perm[j]]++; }
	for (uint64_t i = 0; i < n; i++) CHECK(seen[(size_t)i] == 1, "%s i=%llu", name, (unsigned long long)i);
	std::map<uint32_t, std::vector<uint64_t> > brute;          // b slot -> caller's indices, ascending
	for (uint64_t i = 0; i < n; i++) brute[b_of(i)].push_back(i);
	CHECK(g.runs.size() == brute.size(), "%s runs %zu brute %zu", name, g.runs.size(), brute.size());
	uint64_t at = 0;
	size_t r = 0;
	for (const auto& kv : brute) {
		if (r >= g.runs.size()) break;
		const MscPairRun& run = g.runs[r++];
		CHECK(run.b_slot == kv.first && run.first == at && run.m == kv.second.size(), "%s run %zu", name, r - 1);
		for (uint64_t t = 0; t < run.m && t < kv.second.size(); t++) CHECK(g.perm[(size_t)(run.first + t)] == kv.second[(size_t)t], "%s run %zu entry %llu", name, r - 1, (unsigned long long)t);
		at += kv.second.size();
	}
	CHECK(at == n, "%s", name);
	// chunks: cover [0, n) in order, none empty, none over the budget
	const std::vector<uint64_t> cuts = msc_pair_chunks(n, budget);
	CHECK(!cuts.empty() && cuts.front() == 0 && cuts.back() == n, "%s budget %llu", name, (unsigned long long)budget);
	CHECK(n != 0 || cuts.size() == 1, "%s: no chunk for an empty list", name);
	std::vector<uint64_t> result((size_t)n * 2, ~0ull);          // rows of width 2, caller's order
	std::vector<MscPairRun> runs;
	std::vector<uint32_t> pair_run, cands;
	for (size_t c = 0; c + 1 < cuts.size(); c++) {
		const uint64_t p0 = cuts[c], p1 = cuts[c + 1];
		CHECK(p1 > p0 && p1 - p0 <= (budget ? budget : 1), "%s chunk %zu", name, c);
		uint64_t max_m = 0, covered = 0, longest = 0;
		msc_pair_chunk_runs(g, p0, p1, runs, pair_run, &max_m);
		msc_pair_chunk_a(g, a.data(), p0, p1, cands);
		CHECK(pair_run.size() == p1 - p0 && cands.size() == p1 - p0, "%s chunk %zu", name, c);
		for (size_t s = 0; s < runs.size(); s++) {
			CHECK(runs[s].first == covered && runs[s].m > 0, "%s chunk %zu run %zu", name, c, s);
			CHECK(s == 0 || runs[s - 1].b_slot < runs[s].b_slot, "%s chunk %zu run %zu", name, c, s);
			covered += runs[s].m;
			longest = std::max(longest, runs[s].m);
		}
		CHECK(covered == p1 - p0 && longest == max_m, "%s chunk %zu", name, c);
		// what the device side does: pair j of the chunk = (cands[j], runs[pair_run[j]].b_slot); then scatter
		std::vector<uint64_t> rows((size_t)(p1 - p0) * 2);
		for (uint64_t j = 0; j < p1 - p0; j++) {
			CHECK(pair_run[(size_t)j] < runs.size(), "%s chunk %zu pair %llu", name, c, (unsigned long long)j);
			if (pair_run[(size_t)j] >= runs.size()) continue;
			const MscPairRun& run = runs[pair_run[(size_t)j]];
			CHECK(j >= run.first && j < run.first + run.m, "%s chunk %zu pair %llu", name, c, (unsigned long long)j);
			rows[(size_t)j * 2] = score_of(cands[(size_t)j], run.b_slot);
			rows[(size_t)j * 2 + 1] = p0 + j;
		}
		msc_pair_scatter(g, p0, p1, 2, rows.data(), result.data());
	}
	for (uint64_t i = 0; i < n; i++) CHECK(result[(size_t)i * 2] == score_of(a[(size_t)i], b_of(i)), "%s budget %llu row %llu", name, (unsigned long long)budget, (unsigned long long)i);
	// a_slots == nullptr means slots 0 .. n-1
	if (n) {
		msc_pair_chunk_a(g, nullptr, 0, n, cands);
		for (uint64_t j = 0; j < n; j++) CHECK(cands[(size_t)j] == (uint32_t)g.perm[(size_t)j], "%s identity a", name);
	}
}

int main() {
	const uint64_t budgets[] = {1, 2, 7, 1000};
	std::vector<uint32_t> a, b;
	for (uint64_t budget : budgets) {
		a.clear(); b.clear();
		run_case("n = 0", a, &b, budget);
		a.assign(1, 5); b.assign(1, 9);
		run_case("n = 1", a, &b, budget);
		a.clear(); b.clear();
		for (uint32_t i = 0; i < 23; i++) { a.push_back(100 + i % 5); b.push_back(4); }
		run_case("all-equal b", a, &b, budget);
		a.clear(); b.clear();
		for (uint32_t i = 0; i < 23; i++) { a.push_back(i * 3 % 7); b.push_back(1000 - i * 13); }
		run_case("all-distinct b", a, &b, budget);
		a.clear(); b.clear();
		for (uint32_t i = 0; i < 41; i++) { a.push_back(i % 4); b.push_back((i * 5 + i / 3) % 6); }          // interleaved repeats, repeated pairs
		run_case("interleaved repeats", a, &b, budget);
		run_case("b = identity", a, nullptr, budget);
		uint64_t x = 88172645463325252ull;          // xorshift: a longer random list
		a.clear(); b.clear();
		for (uint32_t i = 0; i < 500; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; a.push_back((uint32_t)(x % 50)); b.push_back((uint32_t)((x >> 20) % 17)); }
		run_case("random", a, &b, budget);
	}
	if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
	printf("pair groups ok\n");
	return 0;
}
