// align_plan_check.cpp -- the launch plans of the alignment kernels (meshclust2_amd/csrc/msc_align_plan.h) held to their own rules on seeded
// lists, without a device: msc_align_plan_full (k_align_pairs, k_align_pairs_dirs), msc_align_plan_banded (k_align_band) and
// msc_align_plan_tiles (a round of k_align_tiles). The needs, rows and cells the checks compare against are written here from msc_align.h,
// msc_align_band.h and msc_align_long.h, not taken from the header under test.
//
//   align_plan_check        prints "align plan ok: ..." and exits 0, or prints the first rule that does not hold and exits 1
//
// Built by tests/test_align_plan_cpu.py with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "msc_align_plan.h"

namespace {

#define CHECK(cond, ...)                                       \
	do {                                                       \
		if (!(cond)) {                                         \
			printf("%s:%d: %s: ", __FILE__, __LINE__, #cond); \
			printf(__VA_ARGS__);                               \
			printf("\n");                                      \
			exit(1);                                           \
		}                                                      \
	} while (0)

const uint32_t kBands[] = {1, 17, 64, 128, 129, 512, 513, kAlignBandNone};

// what the checks hold a plan to: the four quantities of a pair and the key that precedes its LDS class
struct Full {
	static const char* name() { return "full"; }
	static int key(const AlignPair&) { return 4; }
	static uint64_t base(const AlignPair& a) { return msc_align_carry_at(a.la, a.lb); }
	static uint64_t need(const AlignPair& a) { return base(a) + (a.la > 256 ? (uint64_t)(a.lb + 1) * sizeof(MscAlignTriple) : 0); }
	static uint64_t rows(const AlignPair& a) { return (uint64_t)a.lb + 1; }
	static uint64_t cells(const AlignPair& a) { return (uint64_t)a.la * a.lb; }
	static uint64_t plan(std::vector<AlignPair>& p, std::vector<AlignLaunch>& l) { return msc_align_plan_full(p, l); }
};
struct Banded {
	static const char* name() { return "banded"; }
	static int key(const AlignPair& a) { return msc_align_band_cols(msc_align_band_diagonals(a.la, a.lb, a.band)); }
	static uint32_t stripe(const AlignPair& a) { return 64u * (uint32_t)key(a); }
	static uint64_t base(const AlignPair& a) { return msc_align_band_carry_at(a.la, a.lb, stripe(a)); }
	static uint64_t rows(const AlignPair& a) { return a.la > stripe(a) ? msc_align_band_ring(a.la, a.lb, a.band, stripe(a)) : 0; }
	static uint64_t need(const AlignPair& a) { return base(a) + rows(a) * sizeof(MscAlignTriple); }
	static uint64_t cells(const AlignPair& a) { return (uint64_t)a.la * msc_align_band_rows(a.la, a.lb, a.band); }
	static uint64_t plan(std::vector<AlignPair>& p, std::vector<AlignLaunch>& l) { return msc_align_plan_banded(p, l); }
};

template <class S>
int class_of(const AlignPair& a) {
	int c = 0;
	while (c < kAlignClasses - 1 && S::need(a) > kAlignClassTop[c]) c++;
	return c;
}

AlignPair pair_of(uint32_t la, uint32_t lb, uint32_t band) {
	AlignPair a{};
	a.la = la; a.lb = lb; a.band = band;
	return a;
}

// For la and a band, the two lengths lb, lb + 1 that straddle each class top; *exact counts the tops a need meets exactly
template <class S>
void add_class_edges(std::vector<AlignPair>& list, uint32_t la, uint32_t band, int* exact) {
	uint64_t below = S::need(pair_of(la, 1, band));
	for (uint32_t lb = 1; lb < kAlignMaxLen; lb++) {
		const uint64_t above = S::need(pair_of(la, lb + 1, band));
		for (int c = 0; c < kAlignClasses - 1; c++) {
			if (below <= kAlignClassTop[c] && above > kAlignClassTop[c]) {
				list.push_back(pair_of(la, lb, band));
				list.push_back(pair_of(la, lb + 1, band));
				if (below == kAlignClassTop[c]) exact[c]++;
			}
		}
		below = above;
	}
}

template <class S>
std::vector<AlignPair> seeded_list(uint32_t seed, bool cross_scratch) {
	std::mt19937 rng(seed);
	std::vector<AlignPair> list;
	auto band = [&]() { return kBands[rng() % 8]; };
	for (int k = 0; k < 1500; k++) list.push_back(pair_of(1 + rng() % 3000, 1 + rng() % 3000, band()));
	for (int k = 0; k < 60; k++) list.push_back(pair_of(1 + rng() % kAlignMaxLen, 1 + rng() % kAlignMaxLen, band()));
	for (uint32_t la : {1u, 63u, 64u, 65u, 127u, 128u, 129u, 255u, 256u, 257u, 511u, 512u, 513u})
		for (uint32_t lb : {1u, 64u, 300u}) for (uint32_t w : kBands) list.push_back(pair_of(la, lb, w));
	for (int k = 0; k < 40; k++) list.push_back(list[rng() % list.size()]);          // equal elements, apart in the list
	// the edges of every LDS class: a need of exactly kAlignClassTop[c], and the next need above it
	int exact[kAlignClasses - 1] = {0, 0, 0, 0};
	for (uint32_t la : {1u, 200u, 257u, 513u, 769u, 1000u, 1025u, 2049u, 5000u, 20000u, kAlignMaxLen})
		for (uint32_t w : kBands) add_class_edges<S>(list, la, w, exact);
	for (int c = 0; c < kAlignClasses - 1; c++) CHECK(exact[c] > 0, "%s: no pair of the list needs exactly %u bytes", S::name(), kAlignClassTop[c]);
	list.push_back(pair_of(kAlignMaxLen, kAlignMaxLen, kAlignBandNone));          // past kAlignLdsMax: the global carry
	CHECK(S::need(list.back()) > kAlignLdsMax, "%s: the largest pair fits LDS", S::name());
	if (cross_scratch)          // enough global-carry rows for a second launch
		for (int k = 0; k < 700; k++) list.push_back(pair_of(kAlignMaxLen - (uint32_t)(rng() % 3), kAlignMaxLen - (uint32_t)(k % 5), kAlignBandNone));
	for (size_t k = list.size(); k > 1; k--) std::swap(list[k - 1], list[rng() % k]);
	for (size_t k = 0; k < list.size(); k++) { list[k].out = (uint32_t)k; list[k].off1 = 7 * k; list[k].off2 = 11 * k + 1; list[k].carry = 0; }
	return list;
}

// -> global-carry launches
template <class S>
int check_plan(const std::vector<AlignPair>& input, const char* what) {
	std::vector<AlignPair> pairs = input;
	std::vector<AlignLaunch> launches(3);          // (stale entries: the plan clears them)
	const uint64_t scratch_rows = S::plan(pairs, launches);
	const size_t n = pairs.size();
	CHECK(n == input.size(), "%s %s: %zu pairs became %zu", S::name(), what, input.size(), n);
	// a permutation of the input
	std::vector<char> seen(n, 0);
	for (const AlignPair& a : pairs) {
		CHECK(a.out < n && !seen[a.out], "%s %s: pair %u twice or out of range", S::name(), what, a.out);
		seen[a.out] = 1;
		const AlignPair& b = input[a.out];
		CHECK(a.off1 == b.off1 && a.off2 == b.off2 && a.la == b.la && a.lb == b.lb && a.band == b.band, "%s %s: pair %u changed", S::name(), what, a.out);
	}
	// keys do not decrease, cells do not increase inside a key, equal elements keep the input's order
	for (size_t k = 1; k < n; k++) {
		const AlignPair &x = pairs[k - 1], &y = pairs[k];
		const int kx = S::key(x) * kAlignClasses + class_of<S>(x), ky = S::key(y) * kAlignClasses + class_of<S>(y);
		CHECK(kx <= ky, "%s %s: position %zu: key %d after %d", S::name(), what, k, ky, kx);
		if (kx == ky) CHECK(S::cells(x) >= S::cells(y), "%s %s: position %zu: cells grow inside key %d", S::name(), what, k, kx);
		if (kx == ky && S::cells(x) == S::cells(y)) CHECK(x.out < y.out, "%s %s: position %zu: equal pairs %u, %u left the input's order", S::name(), what, k, x.out, y.out);
	}
	// the launches tile [0, n)
	uint64_t at = 0, most_rows = 0;
	int global = 0;
	for (size_t i = 0; i < launches.size(); i++) {
		const AlignLaunch& l = launches[i];
		CHECK(l.at == at && l.n > 0 && l.at + l.n <= n, "%s %s: launch %zu covers [%llu, +%llu), expected from %llu", S::name(), what, i, (unsigned long long)l.at, (unsigned long long)l.n,
		      (unsigned long long)at);
		at += l.n;
		const int key = S::key(pairs[l.at]), cls = class_of<S>(pairs[l.at]);
		CHECK(l.cols == key && l.lds_carry == (cls < kAlignClasses - 1), "%s %s: launch %zu: %d columns, carry in LDS %d for key %d class %d", S::name(), what, i, l.cols, (int)l.lds_carry, key, cls);
		uint64_t lds = 0, rows = 0;
		std::vector<std::pair<uint64_t, uint64_t>> ranges;
		for (uint64_t k = l.at; k < l.at + l.n; k++) {
			const AlignPair& a = pairs[k];
			CHECK(S::key(a) == key && class_of<S>(a) == cls, "%s %s: launch %zu mixes keys", S::name(), what, i);
			lds = std::max(lds, l.lds_carry ? S::need(a) : S::base(a));
			rows += S::rows(a);
			if (!l.lds_carry) ranges.push_back({a.carry, a.carry + S::rows(a)});
		}
		CHECK(l.lds == lds && l.lds <= kAlignLdsMax, "%s %s: launch %zu asks for %u bytes of LDS, its pairs need %llu", S::name(), what, i, l.lds, (unsigned long long)lds);
		if (l.lds_carry) { CHECK(l.rows == 0, "%s %s: launch %zu: rows in an LDS-carry launch", S::name(), what, i); continue; }
		global++;
		CHECK(l.rows == rows && (rows <= kAlignScratchRows || l.n == 1), "%s %s: launch %zu: %llu rows, its pairs use %llu", S::name(), what, i, (unsigned long long)l.rows, (unsigned long long)rows);
		std::sort(ranges.begin(), ranges.end());
		for (size_t k = 0; k < ranges.size(); k++) {
			CHECK(ranges[k].second <= scratch_rows, "%s %s: launch %zu: a carry range ends at %llu of %llu rows", S::name(), what, i, (unsigned long long)ranges[k].second, (unsigned long long)scratch_rows);
			if (k) CHECK(ranges[k - 1].second <= ranges[k].first, "%s %s: launch %zu: carry ranges overlap", S::name(), what, i);
		}
		most_rows = std::max(most_rows, rows);
		// a class is cut in two only where the scratch budget says so
		if (i + 1 < launches.size() && launches[i + 1].at < n && S::key(pairs[launches[i + 1].at]) == key && class_of<S>(pairs[launches[i + 1].at]) == cls)
			CHECK(rows + S::rows(pairs[launches[i + 1].at]) > kAlignScratchRows, "%s %s: launch %zu ends before the budget does", S::name(), what, i);
	}
	CHECK(at == n, "%s %s: the launches cover %llu of %zu pairs", S::name(), what, (unsigned long long)at, n);
	CHECK(scratch_rows == most_rows, "%s %s: %llu scratch rows, the largest launch uses %llu", S::name(), what, (unsigned long long)scratch_rows, (unsigned long long)most_rows);
	for (size_t i = 1; i < launches.size(); i++) {          // LDS-carry classes are never cut
		const AlignPair &x = pairs[launches[i - 1].at], &y = pairs[launches[i].at];
		if (launches[i].lds_carry) CHECK(S::key(x) != S::key(y) || class_of<S>(x) != class_of<S>(y), "%s %s: launches %zu and %zu share an LDS class", S::name(), what, i - 1, i);
	}
	return global;
}

// the rounds of a list at H rows a tile -> rounds
int check_tiles(const std::vector<AlignPair>& input, uint32_t H, const char* what, uint64_t* total_tiles) {
	std::vector<AlignPair> pairs = input;
	AlignTileRound R;
	int rounds = 0;
	size_t at = 0;
	for (; at < pairs.size(); at += R.n, rounds++) {
		msc_align_plan_tiles(pairs, at, H, R);
		CHECK(R.n >= 1 && at + R.n <= pairs.size(), "%s H %u: a round of %zu pairs at %zu", what, H, R.n, at);
		// both budgets, or one pair; and the round stops only where the next pair would pass one
		std::vector<std::vector<uint64_t>> stripe_at(R.n);          // where a stripe's tiles start in the order pair, stripe, block
		std::vector<std::pair<uint64_t, uint64_t>> ranges;
		uint64_t tiles = 0, triples = 0;
		uint32_t launches = 0;
		auto count = [&](const AlignPair& a, std::vector<uint64_t>* where) {
			const MscAlignBand band = msc_align_long_band(a.la, a.lb, a.band);
			uint64_t t = 0;
			for (uint32_t s = 0; s < msc_align_stripes(a.la); s++) {
				const MscAlignWindow win = msc_align_band_window(band, a.la, a.lb, s * 256 + 1, 256);
				if (where) where->push_back(tiles + t);
				t += (win.r1 - 1) / H - (win.r0 - 1) / H + 1;
			}
			return t;
		};
		for (size_t k = 0; k < R.n; k++) {
			const AlignPair& a = pairs[at + k];
			const uint64_t borders = (uint64_t)a.lb + 1 + (uint64_t)msc_align_stripes(a.la) * 257;
			ranges.push_back({a.carry, a.carry + borders});
			triples += borders;
			tiles += count(a, &stripe_at[k]);
			launches = std::max(launches, msc_align_stripes(a.la) + (a.lb - 1) / H);
		}
		CHECK(R.n == 1 || (triples <= kAlignRoundTriples && tiles <= kAlignRoundTiles), "%s H %u round %d: %llu triples, %llu tiles in %zu pairs", what, H, rounds, (unsigned long long)triples,
		      (unsigned long long)tiles, R.n);
		if (at + R.n < pairs.size()) {
			const AlignPair& a = pairs[at + R.n];
			const uint64_t borders = (uint64_t)a.lb + 1 + (uint64_t)msc_align_stripes(a.la) * 257;
			CHECK(triples + borders > kAlignRoundTriples || tiles + count(a, nullptr) > kAlignRoundTiles, "%s H %u round %d ends before a budget does", what, H, rounds);
		}
		CHECK(R.triples == triples, "%s H %u round %d: %llu triples, its pairs use %llu", what, H, rounds, (unsigned long long)R.triples, (unsigned long long)triples);
		std::sort(ranges.begin(), ranges.end());
		for (size_t k = 0; k < ranges.size(); k++) {
			CHECK(ranges[k].second <= R.triples, "%s H %u round %d: borders past the round's triples", what, H, rounds);
			if (k) CHECK(ranges[k - 1].second <= ranges[k].first, "%s H %u round %d: borders overlap", what, H, rounds);
		}
		// the table: every tile the windows allow exactly once, in launch stripe + block; start is the exclusive scan
		CHECK(R.table.size() == tiles && R.launches == launches && R.start.size() == (size_t)launches + 1, "%s H %u round %d: %zu tiles of %llu, %u launches of %u", what, H, rounds,
		      R.table.size(), (unsigned long long)tiles, R.launches, launches);
		CHECK(R.start[0] == 0 && R.start[launches] == tiles, "%s H %u round %d: start runs from %llu to %llu", what, H, rounds, (unsigned long long)R.start[0], (unsigned long long)R.start[launches]);
		std::vector<char> seen(tiles, 0);
		for (uint32_t d = 0; d < launches; d++) {
			CHECK(R.start[d] <= R.start[d + 1], "%s H %u round %d: start decreases at %u", what, H, rounds, d);
			for (uint64_t i = R.start[d]; i < R.start[d + 1]; i++) {
				const AlignTileItem it = R.table[i];
				CHECK(it.pair < R.n, "%s H %u round %d: tile %llu names pair %u of %zu", what, H, rounds, (unsigned long long)i, it.pair, R.n);
				const AlignPair& a = pairs[at + it.pair];
				CHECK(it.stripe < msc_align_stripes(a.la), "%s H %u round %d: tile %llu names stripe %u", what, H, rounds, (unsigned long long)i, it.stripe);
				const MscAlignWindow win = msc_align_band_window(msc_align_long_band(a.la, a.lb, a.band), a.la, a.lb, it.stripe * 256 + 1, 256);
				CHECK(it.block >= (win.r0 - 1) / H && it.block <= (win.r1 - 1) / H, "%s H %u round %d: tile %llu: block %u outside the window", what, H, rounds, (unsigned long long)i, it.block);
				CHECK(it.stripe + it.block == d, "%s H %u round %d: tile (%u, %u) in launch %u", what, H, rounds, it.stripe, it.block, d);
				const uint64_t id = stripe_at[it.pair][it.stripe] + (it.block - (win.r0 - 1) / H);
				CHECK(!seen[id], "%s H %u round %d: tile (%u, %u, %u) twice", what, H, rounds, it.pair, it.stripe, it.block);
				seen[id] = 1;
			}
		}
		*total_tiles += tiles;
	}
	// the rounds consumed the list in order and changed nothing but the carry offsets
	CHECK(at == pairs.size(), "%s H %u: the rounds cover %zu of %zu pairs", what, H, at, pairs.size());
	for (size_t k = 0; k < pairs.size(); k++)
		CHECK(pairs[k].out == input[k].out && pairs[k].la == input[k].la && pairs[k].lb == input[k].lb && pairs[k].band == input[k].band && pairs[k].off1 == input[k].off1, "%s H %u: pair %zu changed",
		      what, H, k);
	return rounds;
}

}  // namespace

int main() {
	uint64_t planned = 0;
	for (uint32_t seed : {1u, 2u, 3u}) {
		const std::vector<AlignPair> full = seeded_list<Full>(seed, seed == 1), banded = seeded_list<Banded>(100 + seed, seed == 1);
		const int g_full = check_plan<Full>(full, "seeded"), g_banded = check_plan<Banded>(banded, "seeded");
		CHECK(g_full >= (seed == 1 ? 2 : 1) && g_banded >= (seed == 1 ? 2 : 1), "seed %u: %d and %d global-carry launches", seed, g_full, g_banded);
		check_plan<Full>(banded, "the banded list");          // (the full plan does not read the bands)
		planned += 2 * full.size() + banded.size();
	}
	for (uint32_t w : kBands) {          // one half-width for the whole list, as msc_align_pairs_banded calls it
		std::vector<AlignPair> list = seeded_list<Banded>(7, false);
		for (AlignPair& a : list) a.band = w;
		check_plan<Banded>(list, "one band");
		planned += list.size();
	}
	check_plan<Full>(std::vector<AlignPair>(), "empty");
	check_plan<Full>(std::vector<AlignPair>(1, pair_of(300, 300, 0)), "one pair");

	// tiles: short pairs at the edges of stripes and row blocks, long ones at narrow bands, and the two budgets
	std::mt19937 rng(11);
	std::vector<AlignPair> small, wide, deep;
	for (uint32_t la : {1u, 255u, 256u, 257u, 512u, 513u, 1500u})
		for (uint32_t lb : {1u, 15u, 16u, 17u, 255u, 256u, 257u, 600u, 4100u})
			for (uint32_t w : {kAlignBandNone, 1u, 17u, 64u, 300u}) small.push_back(pair_of(la, lb, w));
	for (int k = 0; k < 200; k++) small.push_back(pair_of(1 + rng() % 5000, 1 + rng() % 5000, kBands[rng() % 8]));
	for (int k = 0; k < 4; k++) {          // past kAlignMaxLen, the lengths close to each other: the band's diagonals are |la - lb| + 2 w + 1
		const uint32_t la = 40000 + rng() % 1000000;
		small.push_back(pair_of(la, la - rng() % 500, 1 + rng() % 2000));
	}
	// the borders of 18 pairs of 2^20 - 1 bytes at half-width 1 do not fit one round
	for (int k = 0; k < 18; k++) wide.push_back(pair_of(kAlignLongMaxLen, kAlignLongMaxLen - k, 1));
	CHECK(18 * msc_align_long_borders(kAlignLongMaxLen, kAlignLongMaxLen - 17) > kAlignRoundTriples, "the wide list fits one round");
	// one pair whose tiles alone pass kAlignRoundTiles at 16 rows a tile, between two small ones: a round of its own
	deep = {pair_of(257, 300, 17), pair_of(262144, 262400, kAlignBandNone), pair_of(256, 255, kAlignBandNone)};
	for (std::vector<AlignPair>* l : {&small, &wide, &deep}) for (size_t k = 0; k < l->size(); k++) { (*l)[k].out = (uint32_t)k; (*l)[k].off1 = 13 * k; }
	uint64_t tiles = 0;
	int rounds = 0;
	for (uint32_t H : {16u, 256u}) {
		CHECK(check_tiles(small, H, "small", &tiles) == 1, "the small list took more than one round");
		const int r = check_tiles(wide, H, "wide", &tiles);
		CHECK(r >= 2, "the wide list took %d rounds", r);
		rounds += r;
	}
	CHECK(check_tiles(deep, 16, "deep", &tiles) == 3, "the pair past the tile budget did not get a round of its own");
	printf("align plan ok: %llu pairs planned, %llu tiles in %d rounds and more\n", (unsigned long long)planned, (unsigned long long)tiles, rounds);
	return 0;
}
