// msc_align_trace.h -- the back pointers of msc_align_pairs_trace: where a cell's nibble lives, and the walk from the corner
// that turns them into a run-length encoded CIGAR. Written once for the kernels (msc_align_trace.hip) and for host programs that replay them
// (tests/align_trace_schedule_check.cpp). Plain C++: no HIP type in here. The nibble itself is msc_align.h's (msc_align_cell_dir).
//
// Layout of one pair's directions, step-major per stripe: dirs[stripe][t][lane], one 16-bit word per lane and step of k_align_pairs_dirs's
// sweep -- the four nibbles of the lane's four columns at the row it filled in that step -- so the 64 lanes of a step store 128 contiguous
// bytes. Cell (i, j), 1-based, lives at stripe (i - 1) / 256, lane ((i - 1) % 256) / 4, t = (j - 1) + lane, nibble (i - 1) % 4. Words of
// lanes outside their rows and nibbles of columns past la are never read.
#pragma once
#include <stdint.h>

#include "msc_align.h"

constexpr uint64_t kAlignTraceBytes = 2ull << 30;          // direction bytes of one group of pairs (MSC_ALIGN_TRACE_BYTES=n overrides it, per call)
// the ops of a run, BAM's numbers; sequence 1 is the query, sequence 2 the reference. A run is run << 4 | op
constexpr uint32_t kAlignOpIns = 1, kAlignOpDel = 2, kAlignOpEq = 7, kAlignOpDiff = 8;

MSC_HD uint32_t msc_align_trace_steps(uint32_t lb) { return lb + kAlignLanes - 1; }
// 16-bit words of a pair's directions (a multiple of 64: every pair starts on a 128-byte line)
MSC_HD uint64_t msc_align_trace_words(uint32_t la, uint32_t lb) { return (uint64_t)msc_align_stripes(la) * msc_align_trace_steps(lb) * kAlignLanes; }
MSC_HD uint64_t msc_align_trace_word_at(uint32_t lb, uint32_t stripe, uint32_t t, uint32_t lane) { return ((uint64_t)stripe * msc_align_trace_steps(lb) + t) * kAlignLanes + lane; }
MSC_HD uint32_t msc_align_trace_nibble(const uint16_t* dirs, uint32_t lb, uint32_t i, uint32_t j) {
	const uint32_t col = (i - 1) % kAlignStripe, lane = col / kAlignCols;
	return ((uint32_t)dirs[msc_align_trace_word_at(lb, (i - 1) / kAlignStripe, (j - 1) + lane, lane)] >> (4 * (col % kAlignCols))) & 0xfu;
}

// The walk: from the corner (la, lb) in state `state` (what msc_align_final_dir picked) back along the pointers while i > 0
// and j > 0, then along the boundary. The runs come out BACK TO FRONT: sink.run(op, n) is called once per maximal run, last run first.
template <class Sink>
MSC_HD void msc_align_trace_walk(const uint16_t* dirs, const uint8_t* a, const uint8_t* b, uint32_t la, uint32_t lb, uint32_t state, Sink& sink) {
	uint32_t i = la, j = lb, op = 0, run = 0;
	while (i > 0 && j > 0) {
		const uint32_t nib = msc_align_trace_nibble(dirs, lb, i, j);
		uint32_t now;
		if (state == kAlignFromMatch) { now = a[i - 1] == b[j - 1] ? kAlignOpEq : kAlignOpDiff; state = nib & 3u; i--; j--; }
		else if (state == kAlignFromLower) { now = kAlignOpIns; state = nib & kAlignLowerCont ? kAlignFromLower : kAlignFromMatch; i--; }
		else { now = kAlignOpDel; state = nib & kAlignUpperCont ? kAlignFromUpper : kAlignFromMatch; j--; }
		if (now == op) run++;
		else { if (run) sink.run(op, run); op = now; run = 1; }
	}
	// the boundary: i columns that consume sequence 1 or j columns that consume sequence 2 (one of the two is 0)
	const uint32_t edge = i ? kAlignOpIns : kAlignOpDel, n = i + j;
	if (n) {
		if (edge == op) run += n;
		else { if (run) sink.run(op, run); op = edge; run = n; }
	}
	if (run) sink.run(op, run);
}

struct MscAlignTraceCount {
	uint32_t n = 0;
	MSC_HD void run(uint32_t, uint32_t) { n++; }
};
// end: one past the pair's last word in the op list; the walk's runs fill the range from its back, so the list reads forward
struct MscAlignTraceWrite {
	uint32_t* end;
	MSC_HD void run(uint32_t op, uint32_t n) { *--end = n << 4 | op; }
};
