// msc_align_band.h -- the band, the row window of a stripe, the carry ring, the per-lane step and the exactness certificate of
// msc_align_pairs_banded / msc_align_pairs_auto, written once for the kernel (msc_align_band.hip) and for host programs that
// replay its schedule (tests/align_band_schedule_check.cpp). Plain C++: no HIP type in here. The cell update, the boundaries and the final
// choice are msc_align.h's.
//
// For a half-width w the diagonals lo .. hi of the grid are IN BAND, lo = min(0, la - lb) - w, hi = max(0, la - lb) + w (cell (i, j) lies on
// diagonal i - j). In-band cells hold what 4.6e gives them from their three neighbours; every state of every out-of-band cell, boundary cells
// included, is the constant (kAlignDeep, 0). As msc_align.h, the lane's step and the boundaries are templates over the count word W, so that
// msc_align_pairs_long_banded runs the same lines over wide states.
#pragma once
#include "msc_align.h"

constexpr int32_t kAlignDeep = -(1 << 30);               // the score of an out-of-band state: far below anything the recurrence reaches
constexpr uint32_t kAlignBandNone = 0xffffffffu;         // msc_align_pairs_auto's band_used of a pair that went through the full kernel
constexpr uint32_t kAlignBandDefault = 64;               // what first_band = 0 means (profiles/align_band.md)
// columns a lane keeps (1, 2 or 4) by the band's diagonals: narrow bands take narrow stripes, whose row window wastes fewer cells, wide ones
// the cheaper step of four columns (measured: profiles/align_band.md)
constexpr uint32_t kAlignBandOneCol = 128, kAlignBandTwoCols = 512;

struct MscAlignBand {
	int32_t lo, hi;
};

MSC_HD MscAlignBand msc_align_band(uint32_t la, uint32_t lb, uint32_t w) {
	const int32_t ww = w > 2 * kAlignMaxLen ? (int32_t)(2 * kAlignMaxLen) : (int32_t)w, d = (int32_t)la - (int32_t)lb;          // (past either length a band covers the grid)
	MscAlignBand b;
	b.lo = (d < 0 ? d : 0) - ww;
	b.hi = (d > 0 ? d : 0) + ww;
	return b;
}
MSC_HD uint32_t msc_align_band_diagonals(uint32_t la, uint32_t lb, uint32_t w) {
	const MscAlignBand b = msc_align_band(la, lb, w);
	return (uint32_t)(b.hi - b.lo + 1);
}
MSC_HD bool msc_align_in_band(const MscAlignBand& b, int32_t i, int32_t j) { return i - j >= b.lo && i - j <= b.hi; }

MSC_HD MscAlignTriple msc_align_deep() {
	MscAlignTriple t;
	t.m.s = t.l.s = t.u.s = kAlignDeep;
	t.m.w = t.l.w = t.u.w = 0;
	return t;
}
// (the same constant over another count word. As an instantiation of this template the packed one costs k_align_band<4 columns> six VGPRs and a
// wave of occupancy, so the packed one stays a plain function; the overload below picks it)
template <class W>
MSC_HD MscAlignTripleT<W> msc_align_deep(const W*) {
	MscAlignTripleT<W> t;
	t.m.s = t.l.s = t.u.s = kAlignDeep;
	t.m.w = t.l.w = t.u.w = MscAlignCount<W>::of_length(0);
	return t;
}
MSC_HD MscAlignTriple msc_align_deep(const uint32_t*) { return msc_align_deep(); }

// ---------------------------------------------------------------------------------------- the certificate
// true: the banded score s_w proves that the banded triple is the full one. Never true where they differ; it may be
// false where they agree.
MSC_HD bool msc_align_band_certified(uint32_t la, uint32_t lb, uint32_t w, const MscAlignParams& P, int32_t s_w) {
	const int64_t mn = la < lb ? la : lb, d = la < lb ? lb - la : la - lb;
	if ((int64_t)w >= mn) return true;          // no cell is out of band
	const int64_t o = P.open, c = P.cont, smax = P.match > P.mismatch ? P.match : P.mismatch;
	if (o < 0 || c < 0 || smax + 2 * c < 0) return false;          // no certificate is offered
	const int64_t diag = smax * (mn - (int64_t)w - 1);
	const int64_t ub = diag - 2 * o - (2 * (int64_t)w + 2 + d) * c;
	const int64_t few = diag - ((int64_t)w + 1) * c, none = -mn * c;          // (a chain from a boundary state that holds neg_inf: with the most diagonal columns, with none)
	const int64_t pb = (int64_t)msc_align_neg_inf(la, lb, P) + (few > none ? few : none);
	return (int64_t)s_w > (ub > pb ? ub : pb);
}
MSC_HD bool msc_align_band_offered(const MscAlignParams& P) {
	const int32_t smax = P.match > P.mismatch ? P.match : P.mismatch;
	return P.open >= 0 && P.cont >= 0 && smax + 2 * P.cont >= 0;
}

// ---------------------------------------------------------------------------------------- the schedule's sizes
MSC_HD int msc_align_band_cols(uint32_t diagonals) { return diagonals <= kAlignBandOneCol ? 1 : diagonals <= kAlignBandTwoCols ? 2 : 4; }
// rows a stripe of the chosen width sweeps at most
MSC_HD uint32_t msc_align_band_rows(uint32_t la, uint32_t lb, uint32_t w) {
	const uint32_t diagonals = msc_align_band_diagonals(la, lb, w), rows = diagonals + (uint32_t)(kAlignLanes * msc_align_band_cols(diagonals)) - 1;
	return rows < lb ? rows : lb;
}
// msc_align_pairs_auto runs a pair at half-width w only while that fills at most half of the grid's rows per stripe: beyond it the full
// kernel, whose step is cheaper, is as fast and needs no certificate
MSC_HD bool msc_align_band_worth(uint32_t la, uint32_t lb, uint32_t w) {
	const uint32_t mn = la < lb ? la : lb;
	return w < mn && 2 * (uint64_t)msc_align_band_rows(la, lb, w) <= lb;
}

struct MscAlignWindow {
	uint32_t r0, r1;          // the rows a stripe visits, 1-based, both ends included
	int32_t read_hi;          // the last in-band row of the column to the stripe's left
};
// c0: the stripe's first column, 1-based; stripe: its columns
MSC_HD MscAlignWindow msc_align_band_window(const MscAlignBand& b, uint32_t la, uint32_t lb, uint32_t c0, uint32_t stripe) {
	const int32_t c1 = (int32_t)(c0 + stripe - 1 < la ? c0 + stripe - 1 : la), top = (int32_t)c0 - b.hi, bottom = c1 - b.lo, left = (int32_t)c0 - 1 - b.lo;
	MscAlignWindow win;
	win.r0 = top > 1 ? (uint32_t)top : 1u;
	win.r1 = bottom < (int32_t)lb ? (uint32_t)bottom : lb;
	win.read_hi = left < (int32_t)lb ? left : (int32_t)lb;
	return win;
}
MSC_HD uint32_t msc_align_band_stripes(uint32_t la, uint32_t stripe) { return (la + stripe - 1) / stripe; }
// The carry column is a ring: row j of the column a stripe hands on sits at j % ring. A stripe's window has at most `ring` rows, and the
// next stripe reads row j at least 64 steps before the row that takes its place is written
MSC_HD uint32_t msc_align_band_ring(uint32_t la, uint32_t lb, uint32_t w, uint32_t stripe) {
	const uint32_t rows = msc_align_band_diagonals(la, lb, w) + stripe - 1;
	return rows < lb ? rows : lb;
}
// LDS of one pair: the first sequence padded with zeros to whole stripes | pad, the second sequence, pad, rounded up to 8 bytes | the ring
MSC_HD uint32_t msc_align_band_seq2_at(uint32_t la, uint32_t stripe) { return msc_align_band_stripes(la, stripe) * stripe; }
MSC_HD uint32_t msc_align_band_carry_at(uint32_t la, uint32_t lb, uint32_t stripe) { return (msc_align_band_seq2_at(la, stripe) + 2 * kAlignSeqPad + lb + 7u) & ~7u; }
MSC_HD uint32_t msc_align_band_carry_rows(uint32_t la, uint32_t lb, uint32_t w, uint32_t stripe) { return msc_align_band_stripes(la, stripe) > 1 ? msc_align_band_ring(la, lb, w, stripe) : 0; }

// ---------------------------------------------------------------------------------------- a lane of the array
template <int C, class W>
struct MscAlignBandLaneT {
	MscAlignTripleT<W> col[C];      // its C columns at the row it finished last
	MscAlignTripleT<W> prev;        // the column to its left at that row
	uint32_t bytes;                 // its columns' bytes of the first sequence, column c in bits [8c, 8c + 8)
};
template <int C>
using MscAlignBandLane = MscAlignBandLaneT<C, uint32_t>;

// cell (i, r0 - 1), the row above a stripe's window: a boundary cell of row 0 where the window starts at row 1, out of band otherwise (the
// one exception, the column to the left of the stripe, comes from the carry: `from_carry`)
MSC_HD MscAlignTriple msc_align_band_above(const MscAlignBand& b, uint32_t i, uint32_t r0, int32_t neg_inf, const MscAlignParams& P) {
	return r0 == 1 && (int32_t)i <= b.hi ? msc_align_row0(i, neg_inf, P) : msc_align_deep();
}
template <class W>
MSC_HD MscAlignTripleT<W> msc_align_band_above(const MscAlignBand& b, uint32_t i, uint32_t r0, int32_t neg_inf, const MscAlignParams& P, const W* word) {
	return r0 == 1 && (int32_t)i <= b.hi ? msc_align_row0<W>(i, neg_inf, P) : msc_align_deep(word);
}
MSC_HD MscAlignTriple msc_align_band_above(const MscAlignBand& b, uint32_t i, uint32_t r0, int32_t neg_inf, const MscAlignParams& P, const uint32_t*) {
	return msc_align_band_above(b, i, r0, neg_inf, P);
}

// first_col: the 1-based index of the lane's first column; from_carry: cell (first_col - 1, r0 - 1) for the stripe's first lane where r0 > 1
template <int C, class W>
MSC_HD void msc_align_band_lane_init(MscAlignBandLaneT<C, W>& L, const MscAlignBand& b, uint32_t first_col, uint32_t bytes, uint32_t r0, bool first_lane, const MscAlignTripleT<W>& from_carry,
                                     int32_t neg_inf, const MscAlignParams& P) {
	L.prev = first_lane && r0 > 1 ? from_carry : msc_align_band_above(b, first_col - 1, r0, neg_inf, P, (const W*)nullptr);
	for (int c = 0; c < C; c++) L.col[c] = msc_align_band_above(b, first_col + c, r0, neg_inf, P, (const W*)nullptr);
	L.bytes = bytes;
}

// One row: recv = the column to the lane's left at THIS row, byte = the row's byte of the second sequence
template <int C, class W>
MSC_HD void msc_align_band_lane_step(MscAlignBandLaneT<C, W>& L, const MscAlignBand& b, uint32_t first_col, uint32_t row, const MscAlignTripleT<W>& recv, uint32_t byte, const MscAlignParams& P) {
	MscAlignTripleT<W> diag = L.prev, left = recv;
	const int32_t on = (int32_t)first_col - (int32_t)row;          // the diagonal of the lane's first column
	for (int c = 0; c < C; c++) {
		const MscAlignTripleT<W> above = L.col[c];
		msc_align_cell(L.col[c], diag, left, ((L.bytes >> (8 * c)) & 0xffu) == byte, P);
		if (on + c < b.lo || on + c > b.hi) L.col[c] = msc_align_deep((const W*)nullptr);
		diag = above;
		left = L.col[c];
	}
	L.prev = recv;
}

// What the stripe's first lane receives for row `row` (>= 1) of the column to the stripe's left (column c0 - 1): boundary column 0 for the
// first stripe, the carry otherwise (`stored`, read only where the row is in band), out of band past read_hi
template <class W>
MSC_HD MscAlignTripleT<W> msc_align_band_left(const MscAlignWindow& win, bool first_stripe, uint32_t row, const MscAlignTripleT<W>& stored, int32_t neg_inf, const MscAlignParams& P) {
	if ((int32_t)row > win.read_hi) return msc_align_deep((const W*)nullptr);
	return first_stripe ? msc_align_col0<W>(row, neg_inf, P) : stored;
}
