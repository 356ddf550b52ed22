// msc_align_band.hip -- msc_align_pairs_banded and msc_align_pairs_auto on the device: the global alignment of listed pairs over a band of
// diagonals, with a per-pair certificate that the banded integers are the full ones (the band, the window of a stripe, the
// per-lane step and the certificate are msc_align_band.h's, the cell update msc_align.h's).
//
//   k_align_band<columns per lane, carry in LDS> : one pair per wave, the systolic sweep of k_align_pairs with three changes. (1) A stripe of
//       64 * C columns [c0, c1] visits only the rows max(1, c0 - hi) .. min(lb, c1 - lo) that hold an in-band cell of one of its columns; the
//       row above that window is out of band for all of them, so a lane starts from (kAlignDeep, 0) unless the window starts at row 1.
//       (2) After the update a cell that lies outside the band is overwritten with (kAlignDeep, 0). (3) The carry column holds a window's
//       rows only, as a ring of min(lb, diagonals + stripe - 1) rows (row j at j % ring); lane 0 reads (kAlignDeep, 0) for the rows the
//       stripe before did not write, and the one in-band cell above its window, (c0 - 1, c0 - hi - 1), from the ring. The ring lives in LDS
//       behind the sequences, or in the pair's range of the context's scratch buffer when it does not fit.
//   The half-width travels in the pair record, so one call serves pairs of different bands: msc_align_pairs_auto reruns the pairs a round left
//   uncertified with their band doubled, in one group of launches a round, and hands those that a band no longer helps to k_align_pairs.
//   Results go to the pair's own index: no atomics, nothing that depends on the order the waves run in.
//   This file holds the kernel and msc_align_queue_banded, which launches what msc_align_plan_banded (msc_align_plan.h) lists; the entry
//   points and the loop of msc_align_pairs_auto are msc_align_api.hip's.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "msc_objects.h"
#include "msc_align_band.h"
#include "msc_align_host.h"
#include "msc_align_wave.h"

namespace {

template <int C, bool kLdsCarry>
__global__ void __launch_bounds__(kAlignLanes) k_align_band(const uint8_t* __restrict__ text, const AlignPair* __restrict__ pairs, MscAlignParams P, MscAlignTriple* scratch,
                                                            int32_t* __restrict__ score, int32_t* __restrict__ length, int32_t* __restrict__ matches, int32_t* __restrict__ certified) {
	extern __shared__ __attribute__((aligned(16))) unsigned char ab_smem[];
	constexpr uint32_t kStripe = kAlignLanes * C;
	const AlignPair pr = pairs[blockIdx.x];
	const uint32_t lane = threadIdx.x, la = pr.la, lb = pr.lb;
	const uint32_t stripes = msc_align_band_stripes(la, kStripe), seq2_at = msc_align_band_seq2_at(la, kStripe) + kAlignSeqPad;
	const MscAlignBand band = msc_align_band(la, lb, pr.band);
	const uint32_t ring = msc_align_band_ring(la, lb, pr.band, kStripe);
	uint8_t* s1 = ab_smem;
	uint8_t* s2 = ab_smem + seq2_at;
	MscAlignTriple* carry = kLdsCarry ? reinterpret_cast<MscAlignTriple*>(ab_smem + msc_align_band_carry_at(la, lb, kStripe)) : scratch + pr.carry;
	for (uint32_t i = lane; i < stripes * kStripe; i += kAlignLanes) s1[i] = i < la ? text[pr.off1 + i] : (uint8_t)0;
	for (uint32_t i = lane; i < lb + 2 * kAlignSeqPad; i += kAlignLanes) s2[(int32_t)i - (int32_t)kAlignSeqPad] = i >= kAlignSeqPad && i < kAlignSeqPad + lb ? text[pr.off2 + i - kAlignSeqPad] : (uint8_t)0;
	__syncthreads();
	const int32_t neg_inf = msc_align_neg_inf(la, lb, P);
	const MscAlignTriple deep = msc_align_deep();
	MscAlignBandLane<C> L;
	for (uint32_t s = 0; s < stripes; s++) {
		const uint32_t c0 = s * kStripe + 1, first = c0 + lane * C;          // 1-based: the stripe's and the lane's first column
		const MscAlignWindow win = msc_align_band_window(band, la, lb, c0, kStripe);
		const uint32_t steps = win.r1 - win.r0 + kAlignLanes;
		uint32_t bytes = 0;
#pragma unroll
		for (int c = 0; c < C; c++) bytes |= (uint32_t)s1[first - 1 + c] << (8 * c);
		uint32_t rd = win.r0 % ring;                                            // where row r0 sits in the ring
		const MscAlignTriple corner = s && win.r0 > 1 ? carry[rd ? rd - 1 : ring - 1] : deep;          // cell (c0 - 1, r0 - 1)
		msc_align_band_lane_init(L, band, first, bytes, win.r0, lane == 0, corner, neg_inf, P);
		const bool writes = lane == kAlignLanes - 1 && s + 1 < stripes;
		uint32_t wr = rd;                                                       // (the last lane's own count: it writes rows r0, r0 + 1, ...)
		MscAlignTriple out = L.col[C - 1];
		MscAlignTriple next = msc_align_band_left(win, s == 0, win.r0, (int32_t)win.r0 <= win.read_hi && s ? carry[rd] : deep, neg_inf, P);          // what lane 0 receives at the coming step
		for (uint32_t t = 0; t < steps; t++) {
			MscAlignTriple recv = shift_triple(out);
			if (lane == 0) recv = next;
			const uint32_t ahead = win.r0 + t + 1;                              // (one step ahead: the load is under way while this row is filled)
			rd = rd + 1 == ring ? 0 : rd + 1;
			next = msc_align_band_left(win, s == 0, ahead, (int32_t)ahead <= win.read_hi && s ? carry[rd] : deep, neg_inf, P);
			const int32_t row = (int32_t)(win.r0 + t) - (int32_t)lane;          // 1-based
			const uint32_t b = s2[row - 1];
			if (row >= (int32_t)win.r0 && row <= (int32_t)win.r1) {
				msc_align_band_lane_step(L, band, first, (uint32_t)row, recv, b, P);
				if (writes) {
					carry[wr] = L.col[C - 1];
					wr = wr + 1 == ring ? 0 : wr + 1;
				}
			}
			out = L.col[C - 1];
		}
		if (!kLdsCarry) __threadfence();          // the carry rows written in this sweep are read by another lane in the next
	}
	// every lane has ended on row lb: the lane that owns column la reports
	const uint32_t at = (la - 1) % kStripe;
	if (lane == at / C) {
		MscAlignTriple t = L.col[0];
#pragma unroll
		for (int c = 1; c < C; c++) if ((uint32_t)c == at % C) t = L.col[c];
		const MscAlignState r = msc_align_final(t);
		score[pr.out] = r.s;
		length[pr.out] = (int32_t)(r.w >> 16);
		matches[pr.out] = (int32_t)(r.w & 0xffffu);
		certified[pr.out] = msc_align_band_certified(la, lb, pr.band, P, r.s) ? 1 : 0;
	}
}

template <int C>
void launch_band(bool lds_carry, unsigned n, uint32_t lds, hipStream_t stream, const uint8_t* d_text, const AlignPair* d_pairs, const MscAlignParams& P, MscAlignTriple* scratch, int32_t* d_out,
                 uint64_t n_out) {
	if (lds_carry) k_align_band<C, true><<<dim3(n), dim3(kAlignLanes), lds, stream>>>(d_text, d_pairs, P, nullptr, d_out, d_out + n_out, d_out + 2 * n_out, d_out + 3 * n_out);
	else k_align_band<C, false><<<dim3(n), dim3(kAlignLanes), lds, stream>>>(d_text, d_pairs, P, scratch, d_out, d_out + n_out, d_out + 2 * n_out, d_out + 3 * n_out);
}

}  // namespace

// Queues k_align_band for `pairs` (reordered here), each at its own half-width: pair p's integers and its flag go to d_out[p.out],
// d_out[n_out + p.out], d_out[2 * n_out + p.out] and d_out[3 * n_out + p.out]
int msc_align_queue_banded(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out) {
	const uint64_t n_pairs = pairs.size();
	std::vector<AlignLaunch> launches;
	const uint64_t scratch_rows = msc_align_plan_banded(pairs, launches);
	if (int r = ensure(ctx, ctx->align_band_pairs, n_pairs * sizeof(AlignPair))) return r;
	if (scratch_rows) if (int r = ensure(ctx, ctx->align_carry, scratch_rows * sizeof(MscAlignTriple))) return r;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->align_band_pairs.p, pairs.data(), n_pairs * sizeof(AlignPair), hipMemcpyHostToDevice, ctx->stream));
	static bool raised = false;
	if (!raised) {
		for (const void* f : {(const void*)k_align_band<1, true>, (const void*)k_align_band<1, false>, (const void*)k_align_band<2, true>, (const void*)k_align_band<2, false>,
		                      (const void*)k_align_band<4, true>, (const void*)k_align_band<4, false>})
			HIP_TRY(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAlignLdsMax));
		raised = true;
	}
	const AlignPair* d_pairs = (const AlignPair*)ctx->align_band_pairs.p;
	for (const AlignLaunch& l : launches) {
		if (l.lds > kAlignLdsMax) return fail(ctx, MSC_ERR_INVALID_ARG, "k_align_band: a pair needs %u bytes of LDS", l.lds);          // (cannot happen within the length limit)
		MscAlignTriple* scratch = (MscAlignTriple*)ctx->align_carry.p;
		if (l.cols == 1) launch_band<1>(l.lds_carry, (unsigned)l.n, l.lds, ctx->stream, d_text, d_pairs + l.at, P, scratch, d_out, n_out);
		else if (l.cols == 2) launch_band<2>(l.lds_carry, (unsigned)l.n, l.lds, ctx->stream, d_text, d_pairs + l.at, P, scratch, d_out, n_out);
		else launch_band<4>(l.lds_carry, (unsigned)l.n, l.lds, ctx->stream, d_text, d_pairs + l.at, P, scratch, d_out, n_out);
		HIP_TRY(ctx, hipGetLastError());
	}
	snprintf(ctx->last_kernel_buf, sizeof(ctx->last_kernel_buf), "k_align_band<%d column%s a lane, carry in %s>", launches.back().cols, launches.back().cols > 1 ? "s" : "",
	         launches.back().lds_carry ? "LDS" : "global memory");
	ctx->last_kernel = ctx->last_kernel_buf;
	ctx->last_query_tile = 0;
	return MSC_OK;
}
