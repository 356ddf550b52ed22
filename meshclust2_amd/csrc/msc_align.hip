// msc_align.hip -- msc_align_pairs on the device: the global-alignment identity of listed pairs (the definition and the cell
// update are msc_align.h's).
//
//   k_align_pairs<carry in LDS> : one pair per wave (a workgroup is one wave). The wave is a systolic array over the anti-diagonals: lane l keeps
//       kAlignCols consecutive columns of the first sequence in registers and, at step t of a sweep, fills row t - l + 1 of them; its last column's
//       three states (a score word and a length | count word each) reach lane l + 1 for the next step through six DPP wave shifts. A first
//       sequence longer than kAlignStripe columns takes several sweeps: lane 63 writes its column row by row into the CARRY column, which lane 0
//       of the next sweep reads back in place (row j is read 65 steps before it is written again). The carry lives in LDS behind the two
//       sequences while the pair's total fits a workgroup's LDS, otherwise in the pair's own range of a scratch buffer the context owns.
//       Both sequences are staged in LDS as bytes, the first padded with zeros to whole stripes (columns past its end are computed and
//       never read), the second with kAlignSeqPad zeros on either side (a lane's row index runs up to 63 outside it).
//   The host sorts the pairs by cells, longest first, inside classes of LDS need (msc_align_plan.h: msc_align_plan_full; a launch asks for its
//   class's largest need, so short pairs keep their occupancy beside a few long ones); block b of a launch takes the b-th pair of its class.
//   Results go to the pair's own index: no atomics, no reduction, nothing that depends on the order the waves run in.
//   This file holds the kernel and msc_align_queue_full; the entry point, msc_align_pairs, is msc_align_api.hip's.
#include <algorithm>
#include <vector>

#include "msc_objects.h"
#include "msc_align.h"
#include "msc_align_host.h"
#include "msc_align_wave.h"

namespace {

template <bool kLdsCarry>
__global__ void __launch_bounds__(kAlignLanes) k_align_pairs(const uint8_t* __restrict__ text, const AlignPair* __restrict__ pairs, MscAlignParams P, MscAlignTriple* scratch,
                                                             int32_t* __restrict__ score, int32_t* __restrict__ length, int32_t* __restrict__ matches) {
	extern __shared__ __attribute__((aligned(16))) unsigned char al_smem[];
	const AlignPair pr = pairs[blockIdx.x];
	const uint32_t lane = threadIdx.x, la = pr.la, lb = pr.lb;
	const uint32_t stripes = msc_align_stripes(la), seq2_at = msc_align_seq2_at(la) + kAlignSeqPad;
	uint8_t* s1 = al_smem;
	uint8_t* s2 = al_smem + seq2_at;
	MscAlignTriple* carry = kLdsCarry ? reinterpret_cast<MscAlignTriple*>(al_smem + msc_align_carry_at(la, lb)) : scratch + pr.carry;
	for (uint32_t i = lane; i < stripes * kAlignStripe; i += kAlignLanes) s1[i] = i < la ? text[pr.off1 + i] : (uint8_t)0;
	for (uint32_t i = lane; i < lb + 2 * kAlignSeqPad; i += kAlignLanes) s2[(int32_t)i - (int32_t)kAlignSeqPad] = i >= kAlignSeqPad && i < kAlignSeqPad + lb ? text[pr.off2 + i - kAlignSeqPad] : (uint8_t)0;
	__syncthreads();
	const int32_t neg_inf = msc_align_neg_inf(la, lb, P);
	const uint32_t steps = lb + kAlignLanes - 1;
	MscAlignLane L;
	for (uint32_t s = 0; s < stripes; s++) {
		const uint32_t first = s * kAlignStripe + lane * kAlignCols;          // 0-based index of the lane's first column
		msc_align_lane_init(L, first + 1, *reinterpret_cast<const uint32_t*>(s1 + first), neg_inf, P);
		const bool writes = lane == kAlignLanes - 1 && s + 1 < stripes;
		MscAlignTriple out = L.col[kAlignCols - 1];
		MscAlignTriple next = s ? carry[1] : msc_align_col0(1, neg_inf, P);          // what lane 0 receives at the coming step
		for (uint32_t t = 0; t < steps; t++) {
			MscAlignTriple recv = shift_triple(out);
			if (lane == 0) recv = next;
			const uint32_t ahead = t + 2 <= lb ? t + 2 : lb;                 // (one step ahead: the load is under way while this row is filled)
			next = s ? carry[ahead] : msc_align_col0(ahead, neg_inf, P);
			const int32_t row = (int32_t)t - (int32_t)lane;                     // 0-based
			const uint32_t b = s2[row];
			if (row >= 0 && row < (int32_t)lb) {
				msc_align_lane_step(L, recv, b, P);
				if (writes) carry[row + 1] = L.col[kAlignCols - 1];
			}
			out = L.col[kAlignCols - 1];
		}
		if (!kLdsCarry) __threadfence();          // the carry rows written in this sweep are read by another lane in the next
	}
	// every lane has ended on row lb: the lane that owns column la reports
	const uint32_t at = (la - 1) % kAlignStripe;
	if (lane == at / kAlignCols) {
		MscAlignTriple t = L.col[0];
#pragma unroll
		for (int c = 1; c < kAlignCols; c++) if ((uint32_t)c == at % kAlignCols) t = L.col[c];
		const MscAlignState r = msc_align_final(t);
		score[pr.out] = r.s;
		length[pr.out] = (int32_t)(r.w >> 16);
		matches[pr.out] = (int32_t)(r.w & 0xffffu);
	}
}

}  // namespace

// Queues k_align_pairs for `pairs` (reordered here) over the uploaded text: pair p's integers go to d_out[p.out], d_out[n_out + p.out] and
// d_out[2 * n_out + p.out]
int msc_align_queue_full(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out) {
	const uint64_t n_pairs = pairs.size();
	std::vector<AlignLaunch> launches;
	const uint64_t scratch_rows = msc_align_plan_full(pairs, launches);
	if (int r = ensure(ctx, ctx->align_pairs, n_pairs * sizeof(AlignPair))) return r;
	if (scratch_rows) if (int r = ensure(ctx, ctx->align_carry, scratch_rows * sizeof(MscAlignTriple))) return r;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->align_pairs.p, pairs.data(), n_pairs * sizeof(AlignPair), hipMemcpyHostToDevice, ctx->stream));
	static bool raised = false;
	if (!raised) {
		HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_align_pairs<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAlignLdsMax));
		HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_align_pairs<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAlignLdsMax));
		raised = true;
	}
	const AlignPair* d_pairs = (const AlignPair*)ctx->align_pairs.p;
	for (const AlignLaunch& l : launches) {
		if (l.lds > kAlignLdsMax) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_align_pairs: a pair needs %u bytes of LDS", l.lds);          // (cannot happen within the length limit)
		if (l.lds_carry)
			k_align_pairs<true><<<dim3((unsigned)l.n), dim3(kAlignLanes), l.lds, ctx->stream>>>(d_text, d_pairs + l.at, P, nullptr, d_out, d_out + n_out, d_out + 2 * n_out);
		else
			k_align_pairs<false><<<dim3((unsigned)l.n), dim3(kAlignLanes), l.lds, ctx->stream>>>(d_text, d_pairs + l.at, P, (MscAlignTriple*)ctx->align_carry.p, d_out, d_out + n_out, d_out + 2 * n_out);
		HIP_TRY(ctx, hipGetLastError());
	}
	ctx->last_kernel = launches.back().lds_carry ? "k_align_pairs<carry in LDS>" : "k_align_pairs<carry in global memory>";
	ctx->last_query_tile = 0;
	return MSC_OK;
}
