// msc_align_trace.hip -- msc_align_pairs_trace on the device: msc_align_pairs's triples and the alignment itself, a run-length encoded CIGAR
// per pair (the cell update and its decisions are msc_align.h's, the layout of the back pointers and the walk
// msc_align_trace.h's).
//
//   k_align_pairs_dirs<carry in LDS> : k_align_pairs's schedule (msc_align.hip: one pair per wave, four columns a lane, stripes of 256 columns,
//       the same staging and the same carry) with one addition -- at every step a lane stores the four nibbles of the cells it filled as one
//       16-bit word, dirs[stripe][t][lane]: 128 contiguous bytes per wave and step. The lane that owns the corner also reports the state
//       msc_align_final picked.
//   k_align_trace_count / k_align_trace_write : one lane per pair walks the pointers from the corner (msc_align_trace_walk); the first counts
//       the pair's runs, the second writes them back to front into the pair's range of the op list, so the list reads forward.
//   The host deals the call's pairs, in the caller's order, into groups whose direction bytes fit kAlignTraceBytes (MSC_ALIGN_TRACE_BYTES=n,
//   read on every call; a pair above the cap is a group of its own) and runs per group: the forward launches (msc_align_plan_full's classes,
//   longest first), the count, an exclusive scan on the host, the write. The op list of all groups is one device list in the caller's order,
//   kept by the context until the next call. No atomics; a pair's words depend on the pair and the parameters alone.
//   The checks of the call (msc_align_list) and the fan-out of the three integers (msc_align_download) are msc_align_api.hip's, the plan of a
//   group's forward launches msc_align_plan.h's; the group loop, with its own buffers and its timing events, stays here.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "msc_objects.h"
#include "msc_align.h"
#include "msc_align_trace.h"
#include "msc_align_host.h"
#include "msc_align_wave.h"

namespace {

// dirs_at[blockIdx.x]: where the pair's directions start in `dirs`, in 16-bit words. start[pr.out]: the state the walk starts in
template <bool kLdsCarry>
__global__ void __launch_bounds__(kAlignLanes) k_align_pairs_dirs(const uint8_t* __restrict__ text, const AlignPair* __restrict__ pairs, const uint64_t* __restrict__ dirs_at, MscAlignParams P,
                                                                  MscAlignTriple* scratch, uint16_t* __restrict__ dirs, int32_t* __restrict__ score, int32_t* __restrict__ length,
                                                                  int32_t* __restrict__ matches, int32_t* __restrict__ start) {
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
	const uint32_t steps = msc_align_trace_steps(lb);
	uint16_t* mine = dirs + dirs_at[blockIdx.x] + lane;          // this lane's word of step 0 of stripe 0
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
				const uint32_t d = msc_align_lane_step_dir(L, recv, b, P);
				mine[(uint64_t)t * kAlignLanes] = (uint16_t)d;          // t < steps, s < stripes: inside the pair's msc_align_trace_words
				if (writes) carry[row + 1] = L.col[kAlignCols - 1];
			}
			out = L.col[kAlignCols - 1];
		}
		mine += (uint64_t)steps * kAlignLanes;
		if (!kLdsCarry) __threadfence();          // the carry rows written in this sweep are read by another lane in the next
	}
	// every lane has ended on row lb: the lane that owns column la reports
	const uint32_t at = (la - 1) % kAlignStripe;
	if (lane == at / kAlignCols) {
		MscAlignTriple t = L.col[0];
#pragma unroll
		for (int c = 1; c < kAlignCols; c++) if ((uint32_t)c == at % kAlignCols) t = L.col[c];
		uint32_t from;
		const MscAlignState r = msc_align_final_dir(t, from);
		score[pr.out] = r.s;
		length[pr.out] = (int32_t)(r.w >> 16);
		matches[pr.out] = (int32_t)(r.w & 0xffffu);
		start[pr.out] = (int32_t)from;
	}
}

// One lane per pair of the group (in the launches' order: neighbours have similar lengths). counts[pr.out] / ends[pr.out]: the pair's runs,
// and one past its last word in the op list
__global__ void __launch_bounds__(kAlignLanes) k_align_trace_count(const uint8_t* __restrict__ text, const AlignPair* __restrict__ pairs, const uint64_t* __restrict__ dirs_at, uint64_t n,
                                                                   const uint16_t* __restrict__ dirs, const int32_t* __restrict__ start, uint32_t* __restrict__ counts) {
	const uint64_t k = (uint64_t)blockIdx.x * kAlignLanes + threadIdx.x;
	if (k >= n) return;
	const AlignPair pr = pairs[k];
	MscAlignTraceCount sink;
	msc_align_trace_walk(dirs + dirs_at[k], text + pr.off1, text + pr.off2, pr.la, pr.lb, (uint32_t)start[pr.out], sink);
	counts[pr.out] = sink.n;
}

__global__ void __launch_bounds__(kAlignLanes) k_align_trace_write(const uint8_t* __restrict__ text, const AlignPair* __restrict__ pairs, const uint64_t* __restrict__ dirs_at, uint64_t n,
                                                                   const uint16_t* __restrict__ dirs, const int32_t* __restrict__ start, const uint64_t* __restrict__ ends,
                                                                   uint32_t* __restrict__ ops) {
	const uint64_t k = (uint64_t)blockIdx.x * kAlignLanes + threadIdx.x;
	if (k >= n) return;
	const AlignPair pr = pairs[k];
	MscAlignTraceWrite sink{ops + ends[pr.out]};
	msc_align_trace_walk(dirs + dirs_at[k], text + pr.off1, text + pr.off2, pr.la, pr.lb, (uint32_t)start[pr.out], sink);
}

uint64_t trace_cap() {          // read on every call, like the other switches marked so in DESIGN.md 9
	if (const char* v = getenv("MSC_ALIGN_TRACE_BYTES")) {
		const unsigned long long n = strtoull(v, nullptr, 10);
		if (n > 0) return n;
	}
	return kAlignTraceBytes;
}

}  // namespace

extern "C" int msc_align_pairs_trace(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                     int match, int mismatch, int gap_open, int gap_continue, int32_t* score, int32_t* length, int32_t* matches, uint64_t* op_offsets) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (n_pairs == 0) {
		ctx->align_trace_n = 0;
		if (op_offsets) op_offsets[0] = 0;
		return MSC_OK;
	}
	if (!seqs || !offsets || !first || !second || !score || !length || !matches || !op_offsets) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_align_pairs_trace: a NULL argument");
	std::vector<AlignPair> all;
	uint64_t text_bytes = 0;
	if (int r = msc_align_list(ctx, "msc_align_pairs_trace", offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open, gap_continue, all, text_bytes)) return r;
	const MscAlignParams P = msc_align_params(match, mismatch, gap_open, gap_continue);
	// groups: consecutive pairs of the caller's list whose direction bytes fit the cap, so a group's ranges of the op list are consecutive too
	const uint64_t cap_words = trace_cap() / sizeof(uint16_t);
	std::vector<uint64_t> group_at(1, 0);
	uint64_t most_words = 0, most_pairs = 0;
	for (uint64_t p = 0, words = 0; p < n_pairs; p++) {
		const uint64_t w = msc_align_trace_words(all[p].la, all[p].lb);
		if (p > group_at.back() && words + w > cap_words) { group_at.push_back(p); words = 0; }
		words += w;
		most_words = std::max(most_words, words);
		most_pairs = std::max(most_pairs, p + 1 - group_at.back());
	}
	group_at.push_back(n_pairs);
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	ctx->align_trace_n = 0;          // the list of the call before ends here
	if (int r = ensure(ctx, ctx->align_text, text_bytes + 4)) return r;
	if (int r = ensure(ctx, ctx->align_out, 4 * n_pairs * sizeof(int32_t))) return r;
	if (int r = ensure(ctx, ctx->align_trace_idx, n_pairs * (sizeof(uint64_t) + sizeof(uint32_t)))) return r;
	if (int r = ensure(ctx, ctx->align_trace_at, most_pairs * sizeof(uint64_t))) return r;
	if (int r = ensure(ctx, ctx->align_pairs, most_pairs * sizeof(AlignPair))) return r;
	if (int r = ensure(ctx, ctx->align_trace_dirs, most_words * sizeof(uint16_t))) return r;
	static bool raised = false;
	if (!raised) {
		HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_align_pairs_dirs<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAlignLdsMax));
		HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_align_pairs_dirs<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAlignLdsMax));
		raised = true;
	}
	const uint8_t* d_text = (const uint8_t*)ctx->align_text.p;
	int32_t* d_out = (int32_t*)ctx->align_out.p;
	uint64_t* d_ends = (uint64_t*)ctx->align_trace_idx.p;
	uint32_t* d_counts = (uint32_t*)(d_ends + n_pairs);
	const AlignPair* d_pairs = (const AlignPair*)ctx->align_pairs.p;
	const uint64_t* d_at = (const uint64_t*)ctx->align_trace_at.p;
	uint16_t* d_dirs = (uint16_t*)ctx->align_trace_dirs.p;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->align_text.p, seqs, text_bytes, hipMemcpyHostToDevice, ctx->stream));
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all0, ctx->stream));
	ctx->tiles_ms_accum = 0.f; ctx->tiles_launches = 0; ctx->have_timing = false;
	std::vector<uint64_t> ends(n_pairs + 1, 0);          // ends[p + 1]: one past pair p's last word = op_offsets[p + 1]
	std::vector<uint32_t> counts(n_pairs);
	bool lds_carry_last = true;
	for (size_t g = 0; g + 1 < group_at.size(); g++) {
		const uint64_t g0 = group_at[g], n = group_at[g + 1] - g0;
		std::vector<AlignPair> pairs(all.begin() + g0, all.begin() + g0 + n);
		std::vector<uint64_t> at_of(n), at(n);          // by position in the caller's list | in the launches' order
		uint64_t words = 0;
		for (uint64_t k = 0; k < n; k++) { at_of[k] = words; words += msc_align_trace_words(pairs[k].la, pairs[k].lb); }
		std::vector<AlignLaunch> launches;
		const uint64_t scratch_rows = msc_align_plan_full(pairs, launches);
		for (uint64_t k = 0; k < n; k++) at[k] = at_of[pairs[k].out - g0];
		if (scratch_rows) if (int r = ensure(ctx, ctx->align_carry, scratch_rows * sizeof(MscAlignTriple))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->align_pairs.p, pairs.data(), n * sizeof(AlignPair), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->align_trace_at.p, at.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles0, ctx->stream));
		for (const AlignLaunch& l : launches) {
			if (l.lds > kAlignLdsMax) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_align_pairs_trace: a pair needs %u bytes of LDS", l.lds);          // (cannot happen within the length limit)
			if (l.lds_carry)
				k_align_pairs_dirs<true><<<dim3((unsigned)l.n), dim3(kAlignLanes), l.lds, ctx->stream>>>(d_text, d_pairs + l.at, d_at + l.at, P, nullptr, d_dirs, d_out, d_out + n_pairs,
				                                                                                           d_out + 2 * n_pairs, d_out + 3 * n_pairs);
			else
				k_align_pairs_dirs<false><<<dim3((unsigned)l.n), dim3(kAlignLanes), l.lds, ctx->stream>>>(d_text, d_pairs + l.at, d_at + l.at, P, (MscAlignTriple*)ctx->align_carry.p, d_dirs, d_out,
				                                                                                            d_out + n_pairs, d_out + 2 * n_pairs, d_out + 3 * n_pairs);
			HIP_TRY(ctx, hipGetLastError());
			lds_carry_last = l.lds_carry;
		}
		if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_tiles1, ctx->stream));
		const unsigned blocks = (unsigned)((n + kAlignLanes - 1) / kAlignLanes);
		k_align_trace_count<<<dim3(blocks), dim3(kAlignLanes), 0, ctx->stream>>>(d_text, d_pairs, d_at, n, d_dirs, d_out + 3 * n_pairs, d_counts);
		HIP_TRY(ctx, hipGetLastError());
		HIP_TRY(ctx, hipMemcpyAsync(counts.data() + g0, d_counts + g0, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		float ms = 0.f;
		if (ctx->timing && hipEventElapsedTime(&ms, ctx->ev_tiles0, ctx->ev_tiles1) == hipSuccess) { ctx->tiles_ms_accum += ms; ctx->tiles_launches += (int)launches.size(); ctx->have_timing = true; }
		for (uint64_t p = g0; p < g0 + n; p++) ends[p + 1] = ends[p] + counts[p];
		// the list grows group by group: what the groups before wrote moves to the larger buffer
		if (ends[g0 + n] * sizeof(uint32_t) > ctx->align_trace_ops.cap) {
			DevBuf larger;
			if (int r = ensure(ctx, larger, std::max<uint64_t>(ends[g0 + n], ends[g0 + n] / std::max<uint64_t>(g0 + n, 1) * n_pairs) * sizeof(uint32_t))) return r;
			if (ends[g0]) HIP_TRY(ctx, hipMemcpyAsync(larger.p, ctx->align_trace_ops.p, ends[g0] * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
			HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			release(ctx->align_trace_ops);
			ctx->align_trace_ops = larger;
		}
		HIP_TRY(ctx, hipMemcpyAsync(d_ends + g0, ends.data() + g0 + 1, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
		k_align_trace_write<<<dim3(blocks), dim3(kAlignLanes), 0, ctx->stream>>>(d_text, d_pairs, d_at, n, d_dirs, d_out + 3 * n_pairs, d_ends, (uint32_t*)ctx->align_trace_ops.p);
		HIP_TRY(ctx, hipGetLastError());
	}
	if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev_all1, ctx->stream));
	if (int r = msc_align_download(ctx, d_out, n_pairs, score, length, matches, nullptr)) return r;
	std::copy(ends.begin(), ends.end(), op_offsets);
	ctx->align_trace_n = ends[n_pairs];
	ctx->last_kernel = lds_carry_last ? "k_align_pairs_dirs<carry in LDS>" : "k_align_pairs_dirs<carry in global memory>";
	ctx->last_query_tile = 0;
	return MSC_OK;
}

extern "C" int msc_align_pairs_trace_fetch(msc_ctx* ctx, uint64_t first_word, uint64_t n_words, uint32_t* ops) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (first_word > ctx->align_trace_n || n_words > ctx->align_trace_n - first_word)
		return fail(ctx, MSC_ERR_INVALID_ARG, "msc_align_pairs_trace_fetch: words %llu .. %llu of a list of %llu", (unsigned long long)first_word, (unsigned long long)(first_word + n_words),
		            (unsigned long long)ctx->align_trace_n);
	if (n_words == 0) return MSC_OK;
	if (!ops) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_align_pairs_trace_fetch: a NULL argument");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(ops, (const uint32_t*)ctx->align_trace_ops.p + first_word, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MSC_OK;
}
