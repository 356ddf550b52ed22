// msc_align.h -- the cell update, the boundaries and the per-lane step of msc_align_pairs, written once for the kernel
// (msc_align.hip) and for host programs that replay its schedule (tests/align_schedule_check.cpp). Plain C++: no HIP type in here.
//
// The operator is the affine-gap global alignment WITHOUT traceback of the reference's GlobAlignE (utility/GlobAlignE.cpp:123-292): columns
// i = 1 .. la run over the first sequence, rows j = 1 .. lb over the second, and every cell holds three states -- match (both bytes in a column
// of the alignment), lower (a gap that consumes a byte of the first sequence; it moves along the row) and upper (a gap that consumes a byte of
// the second; it moves down the column). A state is a score and, travelling with it, the length of the alignment so far and its identical
// columns; the two counts share one word, length << 16 | count (a listed sequence has at most 32 767 bytes: length <= 65 534, count <= 32 767,
// and the count never carries into the length). msc_align_pairs_long keeps the two counts in a word each, MscAlignWide:
// everything below is a template over that count word W, uint32_t for the packed pair, and is written once for both.
//
//   upper(i, j) = max(match(i, j-1) - (open + cont), upper(i, j-1) - cont)            a tie goes to "opened from match"
//   lower(i, j) = max(match(i-1, j) - (open + cont), lower(i-1, j) - cont)            likewise
//   match(i, j) = s + max(match, lower, upper of (i-1, j-1)), s = match or mismatch    ties: match, then lower, then upper
//   result      = max(match, lower, upper of (la, lb))                                 ties: match, then lower, then upper
//
// The reference has no true minus infinity: the value below, a finite number of the size of real scores, stands in for it, takes part in the
// arithmetic (neg_inf - cont is a legal score) and in the ties (near the corners a true boundary score falls to it or below it).
#pragma once
#include <stdint.h>

#include "msc_layout.h"

constexpr int kAlignLanes = 64;                                  // lanes of the systolic array: one wave
constexpr int kAlignCols = 4;                                    // consecutive columns a lane keeps in registers
constexpr int kAlignStripe = kAlignLanes * kAlignCols;           // columns the wave covers in one sweep over the rows
constexpr uint32_t kAlignMaxLen = 32767;                         // bytes of a listed sequence
constexpr int kAlignMaxParam = 100;                              // |match|, |mismatch|, |gap_open|, |gap_continue|
constexpr uint32_t kAlignSeqPad = 64;                            // zero bytes before and after the second sequence in LDS: a lane's row may lie up to 63 outside it

struct MscAlignParams {
	int32_t match, mismatch, open, cont, open_cont;
	uint32_t w_eq, w_ne;          // what a diagonal step adds to length << 16 | count (the reference counts a column whose SCORE is `match`)
};

struct MscAlignWide {
	uint32_t len, cnt;  // length | identical columns, a word each: sequences of up to kAlignLongMaxLen bytes (msc_align_long.h)
};

template <class W>
struct MscAlignStateT {
	int32_t s;          // score
	W w;                // length << 16 | identical columns (uint32_t), or the two apart (MscAlignWide)
};
using MscAlignState = MscAlignStateT<uint32_t>;

template <class W>
struct MscAlignTripleT {
	MscAlignStateT<W> m, l, u;
};
using MscAlignTriple = MscAlignTripleT<uint32_t>;

MSC_HD MscAlignParams msc_align_params(int match, int mismatch, int gap_open, int gap_continue) {
	MscAlignParams P;
	P.match = match; P.mismatch = mismatch; P.open = gap_open; P.cont = gap_continue; P.open_cont = gap_open + gap_continue;
	P.w_eq = (1u << 16) + 1u;
	P.w_ne = (1u << 16) + (mismatch == match ? 1u : 0u);
	return P;
}

// What the recurrence does to a count word: a boundary state's word, one more column of a gap, one more diagonal column, and the two counts
// as the caller gets them
template <class W> struct MscAlignCount;
template <> struct MscAlignCount<uint32_t> {
	static MSC_HD uint32_t of_length(uint32_t len) { return len << 16; }
	static MSC_HD uint32_t gap(uint32_t w) { return w + (1u << 16); }
	static MSC_HD uint32_t diag(uint32_t w, bool eq, const MscAlignParams& P) { return w + (eq ? P.w_eq : P.w_ne); }
	static MSC_HD uint32_t length(uint32_t w) { return w >> 16; }
	static MSC_HD uint32_t matches(uint32_t w) { return w & 0xffffu; }
};
template <> struct MscAlignCount<MscAlignWide> {
	static MSC_HD MscAlignWide of_length(uint32_t len) { return MscAlignWide{len, 0}; }
	static MSC_HD MscAlignWide gap(MscAlignWide w) { return MscAlignWide{w.len + 1, w.cnt}; }
	static MSC_HD MscAlignWide diag(MscAlignWide w, bool eq, const MscAlignParams& P) { return MscAlignWide{w.len + 1, w.cnt + (eq ? 1u : P.w_ne & 1u)}; }
	static MSC_HD uint32_t length(MscAlignWide w) { return w.len; }
	static MSC_HD uint32_t matches(MscAlignWide w) { return w.cnt; }
};

MSC_HD int32_t msc_align_neg_inf(uint32_t la, uint32_t lb, const MscAlignParams& P) {
	const int32_t shorter = (int32_t)(la < lb ? la : lb), diff = (int32_t)(la < lb ? lb - la : la - lb);
	int32_t v = 0;
	if (diff >= 1) v += -P.open - diff * P.cont;
	return v + P.mismatch * shorter - 1;
}

// column i of row 0 (i = 0: the corner, as row 1 sees it on its diagonal)
template <class W = uint32_t>
MSC_HD MscAlignTripleT<W> msc_align_row0(uint32_t i, int32_t neg_inf, const MscAlignParams& P) {
	MscAlignTripleT<W> t;
	const W w = MscAlignCount<W>::of_length(i);
	t.m.s = i == 0 ? 0 : neg_inf;
	t.u.s = i == 0 ? -P.open : neg_inf;
	t.l.s = i == 0 ? neg_inf : -P.open - (int32_t)i * P.cont;
	t.m.w = t.l.w = t.u.w = w;
	return t;
}

// row r >= 1 of column 0: what column 1 reads to its left (match, lower) and, one row later, on its diagonal (all three)
template <class W = uint32_t>
MSC_HD MscAlignTripleT<W> msc_align_col0(uint32_t r, int32_t neg_inf, const MscAlignParams& P) {
	MscAlignTripleT<W> t;
	t.m.s = t.l.s = neg_inf;
	t.u.s = -P.open - (int32_t)r * P.cont;
	t.m.w = t.l.w = t.u.w = MscAlignCount<W>::of_length(r);
	return t;
}

template <class W>
MSC_HD MscAlignStateT<W> msc_align_gap(const MscAlignStateT<W>& from_match, const MscAlignStateT<W>& from_gap, const MscAlignParams& P) {
	const int32_t a = from_match.s - P.open_cont, b = from_gap.s - P.cont;
	MscAlignStateT<W> r;
	r.s = a >= b ? a : b;
	r.w = MscAlignCount<W>::gap(a >= b ? from_match.w : from_gap.w);
	return r;
}

template <class W>
MSC_HD MscAlignStateT<W> msc_align_diag(const MscAlignTripleT<W>& d, bool eq, const MscAlignParams& P) {
	const int32_t ml = d.m.s >= d.l.s ? d.m.s : d.l.s;
	const W ml_w = d.m.s >= d.l.s ? d.m.w : d.l.w;
	MscAlignStateT<W> r;
	r.s = (ml >= d.u.s ? ml : d.u.s) + (eq ? P.match : P.mismatch);
	r.w = MscAlignCount<W>::diag(ml >= d.u.s ? ml_w : d.u.w, eq, P);
	return r;
}

// col: the cell above (row j - 1) on entry, this cell (row j) on return. diag: column i - 1 at row j - 1. left: column i - 1 at row j (its
// upper state is not read)
template <class W>
MSC_HD void msc_align_cell(MscAlignTripleT<W>& col, const MscAlignTripleT<W>& diag, const MscAlignTripleT<W>& left, bool eq, const MscAlignParams& P) {
	col.u = msc_align_gap(col.m, col.u, P);
	col.m = msc_align_diag(diag, eq, P);
	col.l = msc_align_gap(left.m, left.l, P);
}

template <class W>
MSC_HD MscAlignStateT<W> msc_align_final(const MscAlignTripleT<W>& t) {
	const MscAlignStateT<W> ml = t.m.s >= t.l.s ? t.m : t.l;
	return ml.s >= t.u.s ? ml : t.u;
}

// What a lane of the array holds: its kAlignCols columns at the row it finished last, the column to its left at that row (the diagonal
// of its next row), and its columns' bytes of the first sequence, column c in bits [8c, 8c + 8)
struct MscAlignLane {
	MscAlignTriple col[kAlignCols];
	MscAlignTriple prev;
	uint32_t bytes;
};

// first_col: the 1-based index of the lane's first column
MSC_HD void msc_align_lane_init(MscAlignLane& L, uint32_t first_col, uint32_t bytes, int32_t neg_inf, const MscAlignParams& P) {
	L.prev = msc_align_row0(first_col - 1, neg_inf, P);
	for (int c = 0; c < kAlignCols; c++) L.col[c] = msc_align_row0(first_col + c, neg_inf, P);
	L.bytes = bytes;
}

// One row: recv = the column to the lane's left at THIS row, b = the row's byte of the second sequence. The lane's last column is what it
// hands on
MSC_HD void msc_align_lane_step(MscAlignLane& L, const MscAlignTriple& recv, uint32_t b, const MscAlignParams& P) {
	MscAlignTriple diag = L.prev, left = recv;
	for (int c = 0; c < kAlignCols; c++) {
		const MscAlignTriple above = L.col[c];
		msc_align_cell(L.col[c], diag, left, ((L.bytes >> (8 * c)) & 0xffu) == b, P);
		diag = above;
		left = L.col[c];
	}
	L.prev = recv;
}

// ---------------------------------------------------------------------------------------- the same update, and what it decided
// msc_align_pairs_trace: siblings of the functions above that also return the three `>=` decisions of a cell, its back
// pointers, as a nibble -- bits 0-1 the state that won the diagonal (kAlignFromMatch / Lower / Upper), bit 2 lower CONTINUED (it did not open
// from match), bit 3 upper continued. The states they compute are those of their namesakes, expression for expression.
constexpr uint32_t kAlignFromMatch = 0, kAlignFromLower = 1, kAlignFromUpper = 2;
constexpr uint32_t kAlignLowerCont = 4, kAlignUpperCont = 8;

template <class W>
MSC_HD MscAlignStateT<W> msc_align_gap_dir(const MscAlignStateT<W>& from_match, const MscAlignStateT<W>& from_gap, const MscAlignParams& P, bool& continued) {
	const int32_t a = from_match.s - P.open_cont, b = from_gap.s - P.cont;
	MscAlignStateT<W> r;
	r.s = a >= b ? a : b;
	r.w = MscAlignCount<W>::gap(a >= b ? from_match.w : from_gap.w);
	continued = !(a >= b);
	return r;
}

template <class W>
MSC_HD MscAlignStateT<W> msc_align_diag_dir(const MscAlignTripleT<W>& d, bool eq, const MscAlignParams& P, uint32_t& from) {
	const int32_t ml = d.m.s >= d.l.s ? d.m.s : d.l.s;
	const W ml_w = d.m.s >= d.l.s ? d.m.w : d.l.w;
	MscAlignStateT<W> r;
	r.s = (ml >= d.u.s ? ml : d.u.s) + (eq ? P.match : P.mismatch);
	r.w = MscAlignCount<W>::diag(ml >= d.u.s ? ml_w : d.u.w, eq, P);
	from = ml >= d.u.s ? (d.m.s >= d.l.s ? kAlignFromMatch : kAlignFromLower) : kAlignFromUpper;
	return r;
}

// msc_align_cell, returning the cell's nibble
template <class W>
MSC_HD uint32_t msc_align_cell_dir(MscAlignTripleT<W>& col, const MscAlignTripleT<W>& diag, const MscAlignTripleT<W>& left, bool eq, const MscAlignParams& P) {
	bool upper_cont, lower_cont;
	uint32_t from;
	col.u = msc_align_gap_dir(col.m, col.u, P, upper_cont);
	col.m = msc_align_diag_dir(diag, eq, P, from);
	col.l = msc_align_gap_dir(left.m, left.l, P, lower_cont);
	return from | (lower_cont ? kAlignLowerCont : 0u) | (upper_cont ? kAlignUpperCont : 0u);
}

// msc_align_final, and the state it picked
template <class W>
MSC_HD MscAlignStateT<W> msc_align_final_dir(const MscAlignTripleT<W>& t, uint32_t& from) {
	const MscAlignStateT<W> ml = t.m.s >= t.l.s ? t.m : t.l;
	from = ml.s >= t.u.s ? (t.m.s >= t.l.s ? kAlignFromMatch : kAlignFromLower) : kAlignFromUpper;
	return ml.s >= t.u.s ? ml : t.u;
}

// msc_align_lane_step, returning the nibbles of the lane's kAlignCols cells of the row: column c in bits [4c, 4c + 4)
MSC_HD uint32_t msc_align_lane_step_dir(MscAlignLane& L, const MscAlignTriple& recv, uint32_t b, const MscAlignParams& P) {
	MscAlignTriple diag = L.prev, left = recv;
	uint32_t dirs = 0;
	for (int c = 0; c < kAlignCols; c++) {
		const MscAlignTriple above = L.col[c];
		dirs |= msc_align_cell_dir(L.col[c], diag, left, ((L.bytes >> (8 * c)) & 0xffu) == b, P) << (4 * c);
		diag = above;
		left = L.col[c];
	}
	L.prev = recv;
	return dirs;
}

// ---------------------------------------------------------------------------------------- the schedule's sizes
MSC_HD uint32_t msc_align_stripes(uint32_t la) { return (la + kAlignStripe - 1) / kAlignStripe; }
// LDS of one pair: the first sequence padded with zeros to whole stripes | pad, the second sequence, pad, rounded up to 8 bytes | where the
// carry column lives in LDS, its rows 0 .. lb (24 bytes each; a single stripe has none)
MSC_HD uint32_t msc_align_seq2_at(uint32_t la) { return msc_align_stripes(la) * kAlignStripe; }
MSC_HD uint32_t msc_align_carry_at(uint32_t la, uint32_t lb) { return (msc_align_seq2_at(la) + 2 * kAlignSeqPad + lb + 7u) & ~7u; }
MSC_HD uint32_t msc_align_carry_bytes(uint32_t la, uint32_t lb) { return msc_align_stripes(la) > 1 ? (lb + 1) * (uint32_t)sizeof(MscAlignTriple) : 0; }
