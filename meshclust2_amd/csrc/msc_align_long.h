// msc_align_long.h -- the tiles, the borders and the per-lane start of msc_align_pairs_long / _long_banded / _long_auto, written
// once for the kernel (msc_align_long.hip) and for host programs that replay its schedule (tests/align_long_schedule_check.cpp). Plain C++: no
// HIP type in here. The cell update, the boundaries and the final choice are msc_align.h's, the band, the row window of a stripe, the per-lane
// step and the certificate msc_align_band.h's, both over the wide count word MscAlignWide (length and identical columns in a word each, so
// that neither has a limit below 2^32).
//
// A pair's grid is cut into TILES: stripe s holds the columns 256 s + 1 .. 256 s + 256, row block b the rows b H + 1 .. b H + H, and tile
// (s, b) is the part of that rectangle inside the stripe's row window (msc_align_band_window; the full grid is the band that covers
// everything). One wave fills one tile with the systolic step of k_align_band<4 columns a lane>. Tile (s, b) reads what (s - 1, b), (s, b - 1)
// and (s - 1, b - 1) left behind, so the tiles with s + b = d are independent and launch d runs them all; the order of the launches in the
// stream is the only synchronisation. What a tile leaves behind are two BORDERS in the pair's range of a scratch buffer:
//
//   column border, rows 0 .. lb : entry j is the column to the left of the stripe that reads it, at row j. A tile reads the rows it visits
//       (a step ahead, as k_align_band reads its carry) and its last lane overwrites them in place with the tile's own last column.
//   row border, 257 entries per stripe : entry 1 + k is column k of the stripe at the row above the tile that reads it, entry 0 the cell to the
//       left of the stripe at that row -- the corner of the tile below, which sits in the column border at a row this tile overwrites, so the
//       tile's first lane carries it over. A tile reads the entries when it starts and overwrites them when it ends.
//
// The scratch buffer is never cleared. Whether an entry was written by the tile before, and is in band, is decided by arithmetic on the band
// (msc_align_tile_start, msc_align_band_left) and never by what the entry holds: an entry nobody wrote is never used.
#pragma once
#include "msc_align_band.h"

constexpr uint32_t kAlignLongMaxLen = 1048575;                   // bytes of a sequence listed in a _long call (2^20 - 1; the ranges: DESIGN.md 4.6g)
constexpr uint32_t kAlignTileRows = 256;                         // H, unless MSC_ALIGN_TILE_ROWS says otherwise (profiles/align_long.md)
constexpr uint32_t kAlignTileRowsMin = 16, kAlignTileRowsMax = 32768;
constexpr uint32_t kAlignRowBorder = kAlignStripe + 1;           // entries of a stripe's row border

using MscAlignWideTriple = MscAlignTripleT<MscAlignWide>;
using MscAlignWideLane = MscAlignBandLaneT<kAlignCols, MscAlignWide>;
MSC_HD MscAlignWideTriple msc_align_wide_deep() { return msc_align_deep((const MscAlignWide*)nullptr); }

// msc_align_band without its cap of 2 * kAlignMaxLen: past either length a band covers the grid
MSC_HD MscAlignBand msc_align_long_band(uint32_t la, uint32_t lb, uint32_t w) {
	const int32_t ww = w > 2 * kAlignLongMaxLen ? (int32_t)(2 * kAlignLongMaxLen) : (int32_t)w, d = (int32_t)la - (int32_t)lb;
	MscAlignBand b;
	b.lo = (d < 0 ? d : 0) - ww;
	b.hi = (d > 0 ? d : 0) + ww;
	return b;
}
// msc_align_band_worth for tiles: a band is run only while a stripe's row window is at most half of the grid's rows
MSC_HD bool msc_align_long_worth(uint32_t la, uint32_t lb, uint32_t w) {
	const MscAlignBand b = msc_align_long_band(la, lb, w);
	const uint64_t rows = (uint64_t)(b.hi - b.lo + 1) + kAlignStripe - 1, mn = la < lb ? la : lb;
	return w < mn && 2 * (rows < lb ? rows : lb) <= lb;
}

// a pair's range of the scratch buffer, in triples: the column border, then the row borders stripe by stripe
MSC_HD uint64_t msc_align_long_row_at(uint32_t lb) { return (uint64_t)lb + 1; }
MSC_HD uint64_t msc_align_long_borders(uint32_t la, uint32_t lb) { return msc_align_long_row_at(lb) + (uint64_t)msc_align_stripes(la) * kAlignRowBorder; }

struct MscAlignTile {
	uint32_t c0;                 // the stripe's first column, 1-based
	MscAlignWindow win;          // the stripe's row window
	uint32_t top, bot;           // the tile's rows, 1-based, both ends included
};
// the row blocks that hold a tile of the stripe whose window is `win`
MSC_HD uint32_t msc_align_first_block(const MscAlignWindow& win, uint32_t H) { return (win.r0 - 1) / H; }
MSC_HD uint32_t msc_align_last_block(const MscAlignWindow& win, uint32_t H) { return (win.r1 - 1) / H; }
MSC_HD MscAlignTile msc_align_tile(const MscAlignBand& band, uint32_t la, uint32_t lb, uint32_t stripe, uint32_t block, uint32_t H) {
	MscAlignTile t;
	t.c0 = stripe * kAlignStripe + 1;
	t.win = msc_align_band_window(band, la, lb, t.c0, kAlignStripe);
	const uint32_t first = block * H + 1, last = block * H + H;
	t.top = first > t.win.r0 ? first : t.win.r0;
	t.bot = last < t.win.r1 ? last : t.win.r1;
	return t;
}

// What a lane holds when its tile starts. A tile at the top of its stripe's window starts as a stripe of k_align_band does (row 0 or out of
// band above it; its one in-band neighbour above, cell (c0 - 1, top - 1), still sits in the column border: no tile of this stripe has
// written there). A tile further down takes the row above it from the row border, and entry 0 only where band arithmetic says that the cell
// was computed. col_border / row_border: the pair's column border and the stripe's row border, anything that [] reads an entry of (the kernel's
// pointers; a host replay's checked arrays)
template <class Border>
MSC_HD void msc_align_tile_start(MscAlignWideLane& L, const MscAlignBand& band, const MscAlignTile& t, uint32_t lane, uint32_t bytes, const Border& col_border, const Border& row_border,
                                 int32_t neg_inf, const MscAlignParams& P) {
	const uint32_t first = t.c0 + lane * kAlignCols;
	if (t.top == t.win.r0) {
		const bool stored = lane == 0 && t.c0 > 1 && t.top > 1;
		msc_align_band_lane_init(L, band, first, bytes, t.top, lane == 0, stored ? col_border[t.top - 1] : msc_align_wide_deep(), neg_inf, P);
		return;
	}
	for (int c = 0; c < kAlignCols; c++) L.col[c] = row_border[1 + lane * kAlignCols + c];
	if (lane) L.prev = row_border[lane * kAlignCols];
	else {
		const bool stored = t.c0 > 1 && (int32_t)(t.top - 1) <= t.win.read_hi;
		L.prev = msc_align_band_left(t.win, t.c0 == 1, t.top - 1, stored ? row_border[0] : msc_align_wide_deep(), neg_inf, P);
	}
	L.bytes = bytes;
}

// What the stripe's first lane receives for row `row` of the tile: msc_align_band_left over the column border
template <class Border>
MSC_HD MscAlignWideTriple msc_align_tile_left(const MscAlignTile& t, uint32_t row, const Border& col_border, int32_t neg_inf, const MscAlignParams& P) {
	const bool stored = t.c0 > 1 && (int32_t)row <= t.win.read_hi;
	return msc_align_band_left(t.win, t.c0 == 1, row, stored ? col_border[row] : msc_align_wide_deep(), neg_inf, P);
}
