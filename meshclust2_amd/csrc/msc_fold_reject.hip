// msc_fold_reject.hip -- the integer cut of a folded block (msc_fold_reject.h) on the device (gfx950).
//
//   k_fold_reject_ranges   the minima and maxima the certificate reads, over slots of a set: one thread per slot takes the four scalars of its
//                          record, its second rank moment and the sum of (e - 1) over its list of large bins; a wave folds its 64 and one lane
//                          adds them into the set's ten words with 64-bit atomic min / max. Run by ensure_reject_ranges (msc_mirrors.hip) over
//                          the slots written since: the ranges only ever widen, which keeps them sound.
//   k_fold_reject_cut      one thread per query row of a block, or of a tail group's blocks: T(q), the largest rung of the ladder that certifies
//                          "not close" for every candidate in the ranges with P1' + P2' <= T, or kRejectNoCut. It reads the query's record, moment,
//                          collisions and list, the candidates' ranges and the model; nothing of the product. words[1] counts the rows without a cut.
#include "msc_internal.h"
#include "msc_fold_reject.h"

namespace {

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) { const uint64_t o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
	return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) { const uint64_t o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
	return v;
}

// the sum of (e - 1) over a slot's list of large bins and its largest e (1 without a list); a list longer than the pitch: no bound (2^31 ends every certificate)
__device__ __forceinline__ void list_sums(const uint2* mb, const uint32_t* mb_n, uint32_t pitch, uint64_t slot, uint64_t& g, uint32_t& e_max) {
	const uint32_t n = mb_n[slot];
	g = 0; e_max = 1;
	if (n > pitch) { g = 1ull << 31; e_max = 1u << 20; return; }
	const uint2* l = mb + slot * pitch;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t e = l[i].y;
		g += e ? e - 1 : 0;
		if (e > e_max) e_max = e;
	}
}

__global__ void __launch_bounds__(256) k_fold_reject_ranges(const uint8_t* __restrict__ scalars, uint64_t scalar_stride, const uint2* __restrict__ mb, const uint32_t* __restrict__ mb_n,
                                                            uint32_t pitch, const uint64_t* __restrict__ rk_dev, uint64_t first, uint64_t n, unsigned long long* __restrict__ out) {
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t lo[4] = {~0ull, ~0ull, ~0ull, ~0ull}, hi[4] = {0, 0, 0, 0}, dev = 0, g = 0;
	if (i < n) {
		const uint64_t slot = first + i;
		const MscSlotScalars* s = reinterpret_cast<const MscSlotScalars*>(scalars + slot * scalar_stride);
		lo[0] = hi[0] = s->mag; lo[1] = hi[1] = s->length; lo[2] = hi[2] = s->sum; lo[3] = hi[3] = s->sum_sq;
		dev = rk_dev[slot];
		uint32_t e_max;
		list_sums(mb, mb_n, pitch, slot, g, e_max);
	}
#pragma unroll
	for (int j = 0; j < 4; j++) { lo[j] = wave_min_u64(lo[j]); hi[j] = wave_max_u64(hi[j]); }
	dev = wave_max_u64(dev);
	g = wave_max_u64(g);
	if ((threadIdx.x & 63) == 0) {          // (the order of MscRejectRanges)
#pragma unroll
		for (int j = 0; j < 4; j++) { atomicMin(out + 2 * j, (unsigned long long)lo[j]); atomicMax(out + 2 * j + 1, (unsigned long long)hi[j]); }
		atomicMax(out + 8, (unsigned long long)dev);
		atomicMax(out + 9, (unsigned long long)g);
	}
}

__global__ void __launch_bounds__(128) k_fold_reject_cut(const MscFoldRejectCut a) {
	const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= a.n_out) return;
	int32_t T = kRejectNoCut;
	if (row < a.n_rows) {
		const uint32_t slot = a.q_slots[row];
		const MscSlotScalars* s = reinterpret_cast<const MscSlotScalars*>(a.q_scalars + (uint64_t)slot * a.q_scalar_stride);
		MscRejectQuery q;
		q.mag = s->mag; q.len = s->length; q.sum = s->sum; q.sq = s->sum_sq;
		q.rk_dev = a.q_rk_dev[slot];
		q.x = a.q_x[slot];
		uint64_t g;
		list_sums(reinterpret_cast<const uint2*>(a.q_mb), a.q_mb_n, a.q_pitch, slot, g, q.e_max);
		const MscRejectRanges c = *reinterpret_cast<const MscRejectRanges*>(a.ranges);
		T = msc_fold_reject_cut(*a.model, q, c, a.nbins, a.dtype, a.order);
	}
	a.out[row] = T;
	if (a.words) {          // rows without a cut, once per row of the call: a wave's count in one add
		const uint64_t none = __ballot(row < a.n_rows && T < 0);
		if (none && (threadIdx.x & 63) == (uint32_t)__ffsll((unsigned long long)none) - 1) atomicAdd(a.words + 1, (unsigned long long)__popcll(none));
	}
}

}  // namespace

hipError_t msc_launch_fold_reject_ranges(hipStream_t st, const uint8_t* scalars, uint64_t scalar_stride, const void* mb, const uint32_t* mb_n, uint32_t pitch, const uint64_t* rk_dev,
                                         uint64_t first, uint64_t n, uint64_t* ranges) {
	if (n == 0) return hipSuccess;
	k_fold_reject_ranges<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(scalars, scalar_stride, (const uint2*)mb, mb_n, pitch, rk_dev, first, n, (unsigned long long*)ranges);
	return hipGetLastError();
}

hipError_t msc_launch_fold_reject_cut(hipStream_t st, const MscFoldRejectCut& a) {
	if (a.n_out == 0) return hipSuccess;
	if (a.n_rows > a.n_out || !a.model || !a.ranges || !a.out) return hipErrorInvalidValue;
	k_fold_reject_cut<<<dim3((a.n_out + 127) / 128), dim3(128), 0, st>>>(a);
	return hipGetLastError();
}
