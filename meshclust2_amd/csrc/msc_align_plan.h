// msc_align_plan.h -- the launch plans of the alignment kernels, host only: the pair record, the classes of LDS need, the
// launches of k_align_pairs / k_align_pairs_dirs and of k_align_band, and a round of k_align_tiles with its tile table. Index arithmetic and
// nothing else -- no HIP header, no context -- so that a plain g++ program checks it (tests/align_plan_check.cpp). The geometry it plans over
// is msc_align.h's, msc_align_band.h's and msc_align_long.h's.
#pragma once
#include <algorithm>
#include <vector>

#include "msc_align.h"
#include "msc_align_band.h"
#include "msc_align_long.h"

struct AlignPair {
	uint64_t off1, off2;          // byte offsets of the two sequences in the uploaded text
	uint32_t la, lb;
	uint32_t out;                 // the pair's index in the caller's list
	uint32_t band;                // its half-width (k_align_band, k_align_tiles; k_align_pairs does not read it)
	uint64_t carry;               // offset of its carry range in the scratch buffer, in rows (global-carry launches; k_align_tiles: of its borders)
};

constexpr uint32_t kAlignLdsMax = 160 * 1024;                                       // of a workgroup
constexpr uint32_t kAlignClassTop[] = {8 * 1024, 32 * 1024, 64 * 1024, kAlignLdsMax};          // LDS-carry classes; what needs more keeps its carry in global memory
constexpr int kAlignClasses = 5;
constexpr uint64_t kAlignScratchRows = (512ull << 20) / sizeof(MscAlignTriple);      // carry rows one global-carry launch may use
constexpr uint64_t kAlignRoundTiles = 16ull << 20;          // table entries of one round of k_align_tiles (a single pair may need more: it gets a round of its own)

// One launch of k_align_pairs or k_align_band: pairs [at, at + n) of the sorted list, the dynamic LDS it asks for, the columns a lane keeps
// (4 for the full kernel), where its carry lives and (global carry) the rows of the scratch buffer it uses
struct AlignLaunch { uint64_t at, n; uint32_t lds; int cols; bool lds_carry; uint64_t rows; };

struct AlignTileItem {
	uint32_t pair, stripe, block;
};

// What a kernel's plan is made of. key: what precedes the LDS class in the order (a launch never mixes keys). need: the LDS of a pair that
// keeps its carry there. base: its LDS without the carry. rows: its carry rows in the scratch buffer. cells: what it costs, most first
struct AlignShapeFull {
	static int key(const AlignPair&) { return kAlignCols; }
	static uint64_t need(const AlignPair& a) { return msc_align_carry_at(a.la, a.lb) + msc_align_carry_bytes(a.la, a.lb); }
	static uint32_t base(const AlignPair& a) { return msc_align_carry_at(a.la, a.lb); }
	static uint64_t rows(const AlignPair& a) { return a.lb + 1; }
	static uint64_t cells(const AlignPair& a) { return (uint64_t)a.la * a.lb; }
};
struct AlignShapeBanded {
	static int key(const AlignPair& a) { return msc_align_band_cols(msc_align_band_diagonals(a.la, a.lb, a.band)); }          // columns per lane
	static uint64_t need(const AlignPair& a) { return (uint64_t)base(a) + rows(a) * sizeof(MscAlignTriple); }
	static uint32_t base(const AlignPair& a) { return msc_align_band_carry_at(a.la, a.lb, (uint32_t)(kAlignLanes * key(a))); }
	static uint64_t rows(const AlignPair& a) { return msc_align_band_carry_rows(a.la, a.lb, a.band, (uint32_t)(kAlignLanes * key(a))); }
	static uint64_t cells(const AlignPair& a) { return (uint64_t)a.la * msc_align_band_rows(a.la, a.lb, a.band); }
};

// Sorts `pairs` by key, then class of LDS need (the last class keeps its carry in global memory), most cells first inside each and equal
// ones in the order they came; cuts the launches at the borders of the classes and where a global-carry launch would pass
// kAlignScratchRows; sets the carry offsets. Returns the rows of the scratch buffer the largest launch uses
template <class Shape>
uint64_t msc_align_plan(std::vector<AlignPair>& pairs, std::vector<AlignLaunch>& launches) {
	const uint64_t n_pairs = pairs.size();
	auto class_of = [](const AlignPair& a) {
		const uint64_t need = Shape::need(a);
		int c = 0;
		while (c < kAlignClasses - 1 && need > kAlignClassTop[c]) c++;
		return Shape::key(a) * kAlignClasses + c;
	};
	std::stable_sort(pairs.begin(), pairs.end(), [&](const AlignPair& x, const AlignPair& y) {
		const int cx = class_of(x), cy = class_of(y);
		if (cx != cy) return cx < cy;
		return Shape::cells(x) > Shape::cells(y);
	});
	launches.clear();
	uint64_t scratch_rows = 0;
	for (uint64_t i = 0; i < n_pairs;) {
		const int c = class_of(pairs[i]);
		AlignLaunch l{i, 0, 0, Shape::key(pairs[i]), c % kAlignClasses < kAlignClasses - 1, 0};
		for (; i < n_pairs && class_of(pairs[i]) == c; i++, l.n++) {
			if (l.lds_carry) l.lds = std::max(l.lds, (uint32_t)Shape::need(pairs[i]));
			else {
				const uint64_t rows = Shape::rows(pairs[i]);
				if (l.n && l.rows + rows > kAlignScratchRows) break;
				pairs[i].carry = l.rows;
				l.rows += rows;
				l.lds = std::max(l.lds, Shape::base(pairs[i]));
			}
		}
		scratch_rows = std::max(scratch_rows, l.rows);
		launches.push_back(l);
	}
	return scratch_rows;
}
// k_align_pairs and k_align_pairs_dirs | k_align_band, each pair at its own half-width
inline uint64_t msc_align_plan_full(std::vector<AlignPair>& pairs, std::vector<AlignLaunch>& launches) { return msc_align_plan<AlignShapeFull>(pairs, launches); }
inline uint64_t msc_align_plan_banded(std::vector<AlignPair>& pairs, std::vector<AlignLaunch>& launches) { return msc_align_plan<AlignShapeBanded>(pairs, launches); }

// One round of k_align_tiles: its pairs are [at, at + n) of the list, their borders `triples` entries of the scratch buffer; launch d runs
// the tiles table[start[d]] .. table[start[d + 1]] (pair: its index in the round)
struct AlignTileRound {
	size_t n;
	uint64_t triples;
	uint32_t launches;
	std::vector<AlignTileItem> table;
	std::vector<uint64_t> start;
};

// triples of borders a round may use: the bytes of kAlignScratchRows carry rows
constexpr uint64_t kAlignRoundTriples = kAlignScratchRows * sizeof(MscAlignTriple) / sizeof(MscAlignWideTriple);

// the tiles of a pair at H rows a tile
inline uint64_t msc_align_tiles_of(const AlignPair& a, uint32_t H) {
	const MscAlignBand band = msc_align_long_band(a.la, a.lb, a.band);
	uint64_t n = 0;
	for (uint32_t s = 0; s < msc_align_stripes(a.la); s++) {
		const MscAlignWindow win = msc_align_band_window(band, a.la, a.lb, s * kAlignStripe + 1, kAlignStripe);
		n += msc_align_last_block(win, H) - msc_align_first_block(win, H) + 1;
	}
	return n;
}

// Plans the round that starts at pair `at`: it takes pairs, each at its own half-width (kAlignBandNone: the full grid), while their borders
// fit kAlignRoundTriples and their tiles kAlignRoundTiles -- a pair over either budget is a round of its own --, sets their carry offsets and
// lists their tiles sorted by launch, stripe + row block (count, then place)
inline void msc_align_plan_tiles(std::vector<AlignPair>& pairs, size_t at, uint32_t H, AlignTileRound& R) {
	uint64_t n_tiles = 0;
	R.n = 0;
	R.triples = 0;
	for (; at + R.n < pairs.size(); R.n++) {
		AlignPair& a = pairs[at + R.n];
		const uint64_t need = msc_align_long_borders(a.la, a.lb), t = msc_align_tiles_of(a, H);
		if (R.n && (R.triples + need > kAlignRoundTriples || n_tiles + t > kAlignRoundTiles)) break;
		a.carry = R.triples;
		R.triples += need;
		n_tiles += t;
	}
	R.launches = 0;
	for (size_t k = 0; k < R.n; k++) {
		const AlignPair& a = pairs[at + k];
		R.launches = std::max(R.launches, msc_align_stripes(a.la) + (a.lb - 1) / H);
	}
	R.start.assign((size_t)R.launches + 1, 0);
	R.table.resize(n_tiles);
	for (int pass = 0; pass < 2; pass++) {
		for (size_t k = 0; k < R.n; k++) {
			const AlignPair& a = pairs[at + k];
			const MscAlignBand band = msc_align_long_band(a.la, a.lb, a.band);
			for (uint32_t s = 0; s < msc_align_stripes(a.la); s++) {
				const MscAlignWindow win = msc_align_band_window(band, a.la, a.lb, s * kAlignStripe + 1, kAlignStripe);
				for (uint32_t b = msc_align_first_block(win, H); b <= msc_align_last_block(win, H); b++) {
					if (pass == 0) R.start[s + b + 1]++;
					else R.table[R.start[s + b]++] = AlignTileItem{(uint32_t)k, s, b};
				}
			}
		}
		if (pass == 0) for (uint32_t d = 0; d < R.launches; d++) R.start[d + 1] += R.start[d];
		else { for (uint32_t d = R.launches; d > 0; d--) R.start[d] = R.start[d - 1]; R.start[0] = 0; }          // (placing moved every start to its launch's end)
	}
}
