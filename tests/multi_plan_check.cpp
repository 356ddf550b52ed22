// multi_plan_check.cpp -- stand-alone check of meshclust2_amd/csrc/msc_multi_plan.h (built and run by tests/test_multi_plan_cpu.py with
// -fsanitize=address,undefined): the blocks msc_score_multi cuts its queries into, with and without the matrix cores and with chosen blocks
// declining them, the chunks a block's candidates are cut into, and the stage decisions of a block on the matrix cores (msc_matrix_stages,
// msc_matrix_chunk): every decision switched by each of its conditions alone. Exit status 0 = every case held; a failed check prints its case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// ---- the stage decisions of a block on the matrix cores
// a flags-only, queued, single-chunk block of 128 x 640 whose every decision is "yes": screened, bounds of the distance, folded x 16, piped, own prep stream
static MscMatrixFacts all_yes() {
	MscMatrixFacts f;
	f.model = f.screen_ok = f.close = true;
	f.queued = f.emd_ranks = f.block_pipe = f.emd_bounds = true;
	f.fold_screen = 16;
	f.rk_pitch_c = f.rk_pitch_q = 1024;
	f.moments_c = f.moments_q = f.kbf_c = f.kbf_q = true;
	f.kbf_fold_c = f.kbf_fold_q = 16;
	f.n_q = 128; f.m = f.chunk = 640;
	return f;
}

// the decisions as the issue lists them, condition by condition
static MscMatrixStages by_the_list(const MscMatrixFacts& f) {
	MscMatrixStages s;
	s.screen = f.model && f.screen_ok && (f.close && !f.sum && !f.csum && !f.raw) && !(f.want_div || f.want_grp) && !f.no_screen;
	s.walk_counted = s.screen && f.emd_ranks;
	s.bounds_call = s.walk_counted && f.emd_bounds && !f.emd_decides && f.rk_pitch_c == f.rk_pitch_q && f.moments_c && f.moments_q;
	const uint64_t pairs = f.n_q * f.m;
	s.fold = 0;
	if (s.bounds_call && !f.second_run && f.chunk == f.m && 64 <= pairs && pairs <= 0xffffffffull && !f.fold_overflows && f.kbf_c && f.kbf_fold_c == f.fold_screen && f.kbf_q &&
	    f.kbf_fold_q == f.fold_screen)
		s.fold = f.fold_screen;
	s.piped = f.queued && f.chunk == f.m && !f.div_pass && !f.want_grp && f.block_pipe;
	s.own_prep_stream = s.piped && !f.no_prep;
	s.counted = !f.second_run;
	return s;
}

static bool same(const MscMatrixStages& a, const MscMatrixStages& b) {
	return a.screen == b.screen && a.walk_counted == b.walk_counted && a.bounds_call == b.bounds_call && a.fold == b.fold && a.piped == b.piped && a.own_prep_stream == b.own_prep_stream &&
	       a.counted == b.counted;
}

// one condition changed from all_yes: the decisions named in `off` (s = screen, w = walk_counted, b = bounds_call, f = fold, p = piped, o = own_prep_stream)
// turn off, every other one stays on
template <class Change>
static void stage_case(const char* what, const char* off, Change change) {
	MscMatrixFacts f = all_yes();
	change(f);
	const MscMatrixStages s = msc_matrix_stages(f);
	auto on = [&](char c) { return strchr(off, c) == nullptr; };
	CHECK(s.screen == on('s') && s.walk_counted == on('w') && s.bounds_call == on('b') && s.fold == (on('f') ? 16u : 0u) && s.piped == on('p') && s.own_prep_stream == on('o'),
	      "%s: screen %d walk_counted %d bounds_call %d fold %u piped %d own_prep_stream %d", what, (int)s.screen, (int)s.walk_counted, (int)s.bounds_call, s.fold, (int)s.piped,
	      (int)s.own_prep_stream);
	CHECK(same(s, by_the_list(f)), "%s: not the listed expressions", what);
}

static void stage_cases() {
	const MscMatrixStages yes = msc_matrix_stages(all_yes());
	CHECK(yes.screen && yes.walk_counted && yes.bounds_call && yes.fold == 16 && yes.piped && yes.own_prep_stream && yes.counted, "the all-yes block");
	// screen (and with it everything of the flags-only tail; the pipe does not depend on it)
	stage_case("no model", "swbf", [](MscMatrixFacts& f) { f.model = false; });
	stage_case("screen_ok off", "swbf", [](MscMatrixFacts& f) { f.screen_ok = false; });
	stage_case("no close flags", "swbf", [](MscMatrixFacts& f) { f.close = false; });
	stage_case("sum wanted", "swbf", [](MscMatrixFacts& f) { f.sum = true; });
	stage_case("csum wanted", "swbf", [](MscMatrixFacts& f) { f.csum = true; });
	stage_case("raw wanted", "swbf", [](MscMatrixFacts& f) { f.raw = true; });
	stage_case("MSC_NO_SCREEN", "swbf", [](MscMatrixFacts& f) { f.no_screen = true; });
	stage_case("divergence from cells", "swbf", [](MscMatrixFacts& f) { f.want_div = true; });          // (no pass between the stages: still piped)
	stage_case("divergence from a merge pass", "swbfpo", [](MscMatrixFacts& f) { f.want_div = f.div_pass = true; });
	stage_case("a merge pass alone", "po", [](MscMatrixFacts& f) { f.div_pass = true; });                // (each of the two conditions alone)
	stage_case("group statistic", "swbfpo", [](MscMatrixFacts& f) { f.want_grp = true; });
	// walk_counted
	stage_case("distance not from ranks", "wbf", [](MscMatrixFacts& f) { f.emd_ranks = false; });
	// bounds_call
	stage_case("msc_set_emd_bounds(0)", "bf", [](MscMatrixFacts& f) { f.emd_bounds = false; });
	stage_case("model: emd decides", "bf", [](MscMatrixFacts& f) { f.emd_decides = true; });
	stage_case("unequal pitches", "bf", [](MscMatrixFacts& f) { f.rk_pitch_q = 2048; });
	stage_case("candidates without moments", "bf", [](MscMatrixFacts& f) { f.moments_c = false; });
	stage_case("queries without moments", "bf", [](MscMatrixFacts& f) { f.moments_q = false; });
	// fold
	stage_case("second run", "f", [](MscMatrixFacts& f) { f.second_run = true; });
	CHECK(!msc_matrix_stages([] { MscMatrixFacts f = all_yes(); f.second_run = true; return f; }()).counted, "a second run is not counted again");
	stage_case("model: fold overflows", "f", [](MscMatrixFacts& f) { f.fold_overflows = true; });
	stage_case("candidates without a folded mirror", "f", [](MscMatrixFacts& f) { f.kbf_c = false; });
	stage_case("queries without a folded mirror", "f", [](MscMatrixFacts& f) { f.kbf_q = false; });
	stage_case("candidates folded x 8", "f", [](MscMatrixFacts& f) { f.kbf_fold_c = 8; });
	stage_case("queries folded x 32", "f", [](MscMatrixFacts& f) { f.kbf_fold_q = 32; });
	stage_case("msc_set_fold_screen(0), mirrors of the old fold", "f", [](MscMatrixFacts& f) { f.fold_screen = 0; });
	stage_case("msc_set_fold_screen(8), mirrors of 16", "f", [](MscMatrixFacts& f) { f.fold_screen = 8; });
	{	// every mirror and the switch at another fold: that fold
		MscMatrixFacts f = all_yes();
		f.fold_screen = f.kbf_fold_c = f.kbf_fold_q = 32;
		CHECK(msc_matrix_stages(f).fold == 32, "fold 32");
	}
	stage_case("several chunks", "fpo", [](MscMatrixFacts& f) { f.chunk = 320; });
	// the block's pair count n_q * m: 63, 64, 2^32 - 1, 2^32 (a list of 32-bit pair indices with at least one entry)
	struct { uint64_t n_q, m; bool fits; } counts[] = {{1, 63, false}, {3, 21, false}, {1, 64, true}, {2, 32, true}, {64, 1, true}, {1, 0xffffffffull, true}, {3, 1431655765ull, true},
	                                                   {1, 1ull << 32, false}, {2, 1ull << 31, false}, {128, 1ull << 25, false}, {128, (1ull << 25) - 1, true}};
	for (const auto& cnt : counts) {
		MscMatrixFacts f = all_yes();
		f.n_q = cnt.n_q; f.m = f.chunk = cnt.m;
		const MscMatrixStages s = msc_matrix_stages(f);
		CHECK(s.fold == (cnt.fits ? 16u : 0u) && s.bounds_call && s.piped, "block of %llu x %llu pairs: fold %u", (ull)cnt.n_q, (ull)cnt.m, s.fold);
		CHECK(same(s, by_the_list(f)), "block of %llu x %llu pairs: not the listed expressions", (ull)cnt.n_q, (ull)cnt.m);
		// ... and as a chunk's count n_q * mc (the unfolded decisions: a block of several chunks is never folded)
		f = all_yes();
		f.m = 4 * cnt.m; f.chunk = cnt.m;
		const MscMatrixStages sc = msc_matrix_stages(f);
		const MscMatrixChunk ck = msc_matrix_chunk(sc, cnt.n_q, cnt.m);
		CHECK(sc.bounds_call && sc.fold == 0 && ck.bounds == cnt.fits && ck.open_cap == (cnt.fits ? (uint32_t)(cnt.n_q * cnt.m / 64) : 0u) &&
		          ck.tail == (cnt.fits ? MSC_TAIL_BOUNDS : MSC_TAIL_SCORED),
		      "chunk of %llu x %llu pairs: bounds %d open_cap %u tail %d", (ull)cnt.n_q, (ull)cnt.m, (int)ck.bounds, ck.open_cap, (int)ck.tail);
	}
	// piped / own_prep_stream
	stage_case("not queued", "po", [](MscMatrixFacts& f) { f.queued = false; });
	stage_case("msc_set_block_pipe(0)", "po", [](MscMatrixFacts& f) { f.block_pipe = false; });
	stage_case("MSC_GEMM_NO_PREP", "o", [](MscMatrixFacts& f) { f.no_prep = true; });
	// the three tails
	const MscMatrixChunk folded = msc_matrix_chunk(yes, 128, 640);
	CHECK(folded.bounds && folded.open_cap == 1280 && folded.tail == MSC_TAIL_FOLDED, "folded tail");
	MscMatrixFacts f = all_yes();
	f.second_run = true;
	const MscMatrixChunk second = msc_matrix_chunk(msc_matrix_stages(f), 128, 640);
	CHECK(second.bounds && second.open_cap == 1280 && second.tail == MSC_TAIL_BOUNDS, "bounds tail of a second run");
	f = all_yes();
	f.emd_bounds = false;
	const MscMatrixChunk scored = msc_matrix_chunk(msc_matrix_stages(f), 128, 640);
	CHECK(!scored.bounds && scored.open_cap == 0 && scored.tail == MSC_TAIL_SCORED, "scored tail");
	const MscMatrixChunk odd = msc_matrix_chunk(yes, 72, 601);          // 43 272 pairs: the list's capacity rounds down
	CHECK(odd.bounds && odd.open_cap == 676, "open_cap of 72 x 601");
	// every combination of the conditions of one decision at a time is the listed expression too (the pipe's five facts, the screen's nine)
	for (unsigned bits = 0; bits < 32; bits++) {
		MscMatrixFacts g = all_yes();
		g.queued = bits & 1; g.block_pipe = bits & 2; g.div_pass = bits & 4; g.want_grp = bits & 8; g.no_prep = bits & 16;
		CHECK(same(msc_matrix_stages(g), by_the_list(g)), "pipe facts %u", bits);
	}
	for (unsigned bits = 0; bits < 512; bits++) {
		MscMatrixFacts g = all_yes();
		g.model = bits & 1; g.screen_ok = bits & 2; g.close = bits & 4; g.sum = bits & 8; g.csum = bits & 16; g.raw = bits & 32; g.want_div = bits & 64; g.want_grp = bits & 128;
		g.no_screen = bits & 256;
		CHECK(same(msc_matrix_stages(g), by_the_list(g)), "screen facts %u", bits);
	}
}

int main() {
	stage_cases();
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
