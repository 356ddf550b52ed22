// multi_plan_check.cpp -- stand-alone check of meshclust2_amd/csrc/msc_multi_plan.h (built and run by tests/test_multi_plan_cpu.py with
// -fsanitize=address,undefined): the blocks msc_score_multi cuts its queries into, with and without the matrix cores and with chosen blocks
// declining them, and the chunks a block's candidates are cut into. Exit status 0 = every case held; a failed check prints its case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <set>
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

// declining: the blocks of 128 (by index) that decline the matrix cores
static void plan_case(uint64_t n_q, bool kb_fit, const std::set<uint64_t>& declining) {
	std::vector<MscMultiBlock> blocks(3, MscMultiBlock{7, 7, true});          // (the plan clears what it is handed)
	std::vector<uint64_t> asked;
	msc_multi_plan(n_q, kb_fit, [&](uint64_t q0, uint64_t nq) {
		asked.push_back(q0);
		CHECK(kb_fit && q0 % 128 == 0 && nq >= 2 && nq == std::min<uint64_t>(128, n_q - q0), "n_q %llu: asked about [%llu, +%llu)", (ull)n_q, (ull)q0, (ull)nq);
		return declining.count(q0 / 128) != 0;
	}, blocks);
	// consecutive, cover [0, n_q) once
	uint64_t at = 0;
	for (const MscMultiBlock& b : blocks) {
		CHECK(b.q0 == at && b.nq >= 1, "n_q %llu kb_fit %d: block at %llu of %llu, expected at %llu", (ull)n_q, (int)kb_fit, (ull)b.q0, (ull)b.nq, (ull)at);
		at = b.q0 + b.nq;
	}
	CHECK(at == n_q, "n_q %llu kb_fit %d: covered %llu", (ull)n_q, (int)kb_fit, (ull)at);
	// the sizes, against the rule written out block by block
	size_t i = 0, n_asked = 0;
	const uint64_t blk = kb_fit ? 128 : 64;
	for (uint64_t q0 = 0; q0 < n_q; q0 += blk) {
		const uint64_t nq = std::min(blk, n_q - q0);
		const bool offered = kb_fit && nq >= 2;          // (a single query is never offered: the product takes two and up)
		if (offered) n_asked++;
		if (offered && !declining.count(q0 / 128)) {
			CHECK(i < blocks.size() && blocks[i].q0 == q0 && blocks[i].nq == nq && blocks[i].matrix, "n_q %llu: matrix block at %llu", (ull)n_q, (ull)q0);
			i++;
			continue;
		}
		for (uint64_t s = 0; s < nq; s += 64, i++)          // off the matrix cores: sub-blocks of 64, the last one short -- a trailing single query included
			CHECK(i < blocks.size() && blocks[i].q0 == q0 + s && blocks[i].nq == std::min<uint64_t>(64, nq - s) && !blocks[i].matrix, "n_q %llu kb_fit %d: block at %llu", (ull)n_q,
			      (int)kb_fit, (ull)(q0 + s));
	}
	CHECK(i == blocks.size(), "n_q %llu kb_fit %d: %zu blocks, expected %zu", (ull)n_q, (int)kb_fit, blocks.size(), i);
	CHECK(asked.size() == n_asked, "n_q %llu kb_fit %d: asked %zu times, expected %zu", (ull)n_q, (int)kb_fit, asked.size(), n_asked);
	if (n_q <= blk) CHECK(blocks.size() == (kb_fit && n_q > 64 && declining.count(0) ? 2u : 1u), "n_q %llu kb_fit %d: a call of one block", (ull)n_q, (int)kb_fit);
}

static void chunk_case(uint64_t m, uint64_t cap) {
	const MscCandChunks c = msc_cand_chunks(m, cap);
	CHECK(c.chunk >= 1 && c.n >= 1, "m %llu cap %llu", (ull)m, (ull)cap);
	if (c.chunk < 1 || c.n < 1) return;
	CHECK(c.chunk <= std::max<uint64_t>(cap, 256) || c.chunk == m, "m %llu cap %llu chunk %llu", (ull)m, (ull)cap, (ull)c.chunk);
	CHECK(c.n * c.chunk >= m && m > (c.n - 1) * c.chunk, "m %llu cap %llu chunk %llu n %llu", (ull)m, (ull)cap, (ull)c.chunk, (ull)c.n);
	const uint64_t c0 = std::min(std::max<uint64_t>(cap, 256), m), n = (m + c0 - 1) / c0, chunk = (m + n - 1) / n;          // the three-line formula
	CHECK(c.chunk == chunk && c.n == n, "m %llu cap %llu: chunk %llu n %llu, formula %llu %llu", (ull)m, (ull)cap, (ull)c.chunk, (ull)c.n, (ull)chunk, (ull)n);
}

int main() {
	const uint64_t n_qs[] = {1, 2, 63, 64, 65, 127, 128, 129, 130, 256, 257, 1000};
	const std::set<uint64_t> none, first = {0}, second = {1}, last_of_1000 = {7}, some = {0, 2, 3, 7}, all = {0, 1, 2, 3, 4, 5, 6, 7};
	for (uint64_t n_q : n_qs) {
		plan_case(n_q, false, none);
		for (const std::set<uint64_t>* d : {&none, &first, &second, &last_of_1000, &some, &all}) plan_case(n_q, true, *d);
	}
	const uint64_t ms[] = {1, 255, 256, 257, 6250, 35001, 1000000};
	for (uint64_t m : ms) {
		for (uint64_t cap = 1; cap <= (1ull << 31); cap *= 2)
			for (uint64_t d : {0ull, 1ull, 2ull}) { chunk_case(m, cap + d); if (cap > d) chunk_case(m, cap - d); }
		for (uint64_t cap : {255ull, 300ull, 1000ull, 6249ull, 6250ull, 6251ull, 35000ull, 999999ull, 1000001ull, (1ull << 31)}) chunk_case(m, cap);
	}
	if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
	printf("multi plan ok\n");
	return 0;
}
