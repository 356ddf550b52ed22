// msc_emd_list.hip -- the earth mover's distance of the Q x M close-flag pass WITHOUT the dense rank walk (gfx950).
//
// msc_emd_ranks.hip forms emd(a, b) = sum_t | a_t - b_t | over the padded rows of the ranks mirror for every pair of a block. The close
// flag of almost every pair does not depend on the exact value: with base_t = floor(t * 4^k / pitch) (k_ranks16_build's) the triangle
// inequality gives, exactly in integers, for two rows of ONE pitch
//     | sum_t a_t - sum_t b_t |  <=  emd(a, b)  <=  sum_t | a_t - base_t | + sum_t | b_t - base_t |
// so two moments per slot bound it, and the screen (pair_features.hip, k_pair_epilogue_bits_bound) decides the flag from the interval.
//
//   k_rank_moments      one wave per slot: rk_sum = sum_t a_t, rk_dev = sum_t | a_t - base_t | over the whole padded row. Launched wherever
//                       the ranks mirror is built or refreshed, over the same slots.
//   k_emd_ranks_list    the pairs the interval leaves undecided arrive as a device list of pair indices (q * m_per_query + ci); one wave
//                       per listed pair walks the two rows (v_sad_u16 over the 16-bit form when both sets have it, v_sad_u32 otherwise) and
//                       writes the exact distance. The count is read on the device: no host round trip between the screen and the walk.
#include <algorithm>

#include "msc_internal.h"
#include "msc_kbits.h"

namespace {

typedef int v4i_ __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

__global__ void __launch_bounds__(256) k_rank_moments(const uint32_t* __restrict__ ranks, uint64_t pitch, uint64_t nbins, uint64_t first_slot, uint64_t n_slots,
                                                      uint64_t* __restrict__ rk_sum, uint64_t* __restrict__ rk_dev) {
	const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63;
	if (i >= n_slots) return;
	const uint64_t slot = first_slot + i;
	const uint32_t* row = ranks + slot * pitch;
	uint64_t s = 0, d = 0;
	for (uint64_t t = lane; t < pitch; t += 64) {
		const int64_t a = row[t], base = (int64_t)(t * nbins / pitch);
		s += (uint64_t)a;
		d += (uint64_t)(a > base ? a - base : base - a);
	}
	s = wave_sum_u64(s);
	d = wave_sum_u64(d);
	if (lane == 0) { rk_sum[slot] = s; rk_dev[slot] = d; }
}

// words[0] = pairs appended, words[1] = the overflow word (an append found the list full: the block's flags come from the dense walk, and
// nothing here is needed). Rounds of 1 024 ranks, as the dense kernels take them: a lane's terms of a round fit 32 bits (16 of <= 2^20),
// the rounds add up in 64.
template <bool kU16>
__global__ void __launch_bounds__(256) k_emd_ranks_list(const void* __restrict__ c_rk, const void* __restrict__ q_rk, uint64_t pitch, const uint32_t* __restrict__ cand_slots, uint64_t first,
                                                        uint32_t m_per_query, const uint32_t* __restrict__ q_slots, const uint32_t* __restrict__ list, const uint32_t* __restrict__ words,
                                                        uint32_t cap, uint64_t* __restrict__ emd_list, const MscListGroup g) {
	// (a group of blocks, msc_tail_groups: blockIdx.y is the block; its query slots, list, words and distances lie that many strides on -- all 0 for one block)
	q_slots += (uint64_t)blockIdx.y * g.q_stride; list += blockIdx.y * g.list_stride; words += (uint64_t)blockIdx.y * g.words_stride; emd_list += blockIdx.y * g.list_stride;
	if (words[1]) return;
	const uint32_t n = words[0] < cap ? words[0] : cap;
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
	for (uint32_t i = wave0; i < n; i += gridDim.x * 4) {
		const uint32_t idx = list[i], q = idx / m_per_query, ci = idx % m_per_query;
		const uint64_t c_slot = cand_slots ? cand_slots[ci] : first + ci, q_slot = q_slots[q];
		uint64_t total = 0;
		if constexpr (kU16) {          // pitch is a multiple of 1 024 here; lane l: reduced ranks 512 j + 8 l .. + 7 of the round, two per register
			const uint16_t *a = reinterpret_cast<const uint16_t*>(c_rk) + c_slot * pitch, *b = reinterpret_cast<const uint16_t*>(q_rk) + q_slot * pitch;
			for (uint64_t base = 0; base < pitch; base += 1024) {
				uint32_t t = 0;
#pragma unroll
				for (int j = 0; j < 2; j++) {
					const v4i_ x = *reinterpret_cast<const v4i_*>(a + base + 512 * j + 8 * lane), y = *reinterpret_cast<const v4i_*>(b + base + 512 * j + 8 * lane);
					asm("v_sad_u16 %0, %1, %2, %0" : "+v"(t) : "v"(x.x), "v"(y.x));
					asm("v_sad_u16 %0, %1, %2, %0" : "+v"(t) : "v"(x.y), "v"(y.y));
					asm("v_sad_u16 %0, %1, %2, %0" : "+v"(t) : "v"(x.z), "v"(y.z));
					asm("v_sad_u16 %0, %1, %2, %0" : "+v"(t) : "v"(x.w), "v"(y.w));
				}
				total += t;
			}
		} else {          // pitch is a multiple of 256; lane l: ranks 256 j + 4 l .. + 3 of the round
			const uint32_t *a = reinterpret_cast<const uint32_t*>(c_rk) + c_slot * pitch, *b = reinterpret_cast<const uint32_t*>(q_rk) + q_slot * pitch;
			for (uint64_t base = 0; base < pitch; base += 1024) {
				uint32_t t = 0;
#pragma unroll
				for (int j = 0; j < 4; j++) {
					if (base + 256 * j >= pitch) break;
					const v4i_ x = *reinterpret_cast<const v4i_*>(a + base + 256 * j + 4 * lane), y = *reinterpret_cast<const v4i_*>(b + base + 256 * j + 4 * lane);
					asm("v_sad_u32 %0, %1, %2, %0" : "+v"(t) : "v"(x.x), "v"(y.x));
					asm("v_sad_u32 %0, %1, %2, %0" : "+v"(t) : "v"(x.y), "v"(y.y));
					asm("v_sad_u32 %0, %1, %2, %0" : "+v"(t) : "v"(x.z), "v"(y.z));
					asm("v_sad_u32 %0, %1, %2, %0" : "+v"(t) : "v"(x.w), "v"(y.w));
				}
				total += t;
			}
		}
		total = wave_sum_u64(total);
		if (lane == 0) emd_list[i] = total;
	}
}

// The listed pairs of a FOLDED block (msc_fold.h): the product gave upper bounds of P1 (shared k-mers) and P2 (sum of e_q - 1 over the query's
// large bins the candidate holds), and the list epilogue needs them exact. One wave per listed pair walks the candidate's row of the 32-bit ranks
// mirror -- its k-mers as LOGICAL bins in order, a bin repeated per copy, padded with 4^k --, takes each distinct bin once, reads the query's two
// bits at the bin's physical position from the transposed planes (plane 0: the query holds the k-mer; plane 1: more than once, and its own list
// of large bins has the count), and stores P1 into slice 0 of the product's output (zeros into the other slices) and P2 beside it.
__global__ void __launch_bounds__(256) k_fold_exact_list(const MscFoldExact a_, const MscListGroup g) {
	MscFoldExact a = a_;          // (a group of blocks, as k_emd_ranks_list takes it: the block's offsets once, wave-uniform)
	a.q_slots += (uint64_t)blockIdx.y * g.q_stride; a.list += blockIdx.y * g.list_stride; a.words += (uint64_t)blockIdx.y * g.words_stride;
	a.qT += blockIdx.y * g.qt_stride;
	a.out_min = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(a.out_min) + blockIdx.y * g.min_stride);
	if (a.out_diff) a.out_diff = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(a.out_diff) + blockIdx.y * g.diff_stride);
	if (a.words[1]) return;
	const uint32_t n = a.words[0] < a.cap ? a.words[0] : a.cap;
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
	const uint32_t* qt = reinterpret_cast<const uint32_t*>(a.qT);
	for (uint32_t i = wave0; i < n; i += gridDim.x * 4) {
		const uint32_t idx = a.list[i], q = idx / a.m_per_query, ci = idx % a.m_per_query;
		const uint64_t c_slot = a.cand_slots ? a.cand_slots[ci] : a.first + ci, q_slot = a.q_slots[q];
		const uint32_t* row = a.c_ranks + c_slot * a.pitch;
		const uint2* qmb = reinterpret_cast<const uint2*>(a.q_mb) + q_slot * a.q_pitch;
		const uint32_t q_n = a.q_mb_n[q_slot] < a.q_pitch ? a.q_mb_n[q_slot] : a.q_pitch;
		uint64_t p1 = 0, p2 = 0;
		for (uint64_t t = lane; t < a.pitch; t += 64) {
			const uint32_t bin = row[t];
			if (bin >= a.nbins || (t && row[t - 1] == bin)) continue;          // padding; a further copy of the bin before
			const uint32_t ph = (uint32_t)msc_phys_index(bin, a.E, a.R);
			if (!((qt[msc_qt_word(ph, 0, q, a.qn)] >> (q & 31)) & 1u)) continue;
			p1++;
			if ((qt[msc_qt_word(ph, 1, q, a.qn)] >> (q & 31)) & 1u)
				for (uint32_t j = 0; j < q_n; j++) if (qmb[j].x == ph) { p2 += qmb[j].y - 1; break; }
		}
		p1 = wave_sum_u64(p1);
		p2 = wave_sum_u64(p2);
		if (lane < a.slices) a.out_min[((uint64_t)lane * a.m_per_query + ci) * a.qn + q] = lane ? 0 : (int32_t)p1;
		if (lane == 0 && a.out_diff) a.out_diff[(uint64_t)ci * a.qn + q] = (int32_t)p2;
	}
}

// Behind a block's kernels: its count and overflow word go into the call's totals (totals[0] += pairs walked from the list, totals[1] +=
// blocks whose list overflowed) and are cleared for the next block.
// fold_flag: the block's product was folded (msc_api_multi.hip). An overflow of ITS list is no dense block: totals[2] counts it and the flag tells the
// host, when the call's blocks are through, to score the block again with the true product.
// n_blocks > 1: the lists of a group's blocks (msc_tail_groups), one after the other in block order, so that the totals add up in the order of per-block launches.
__global__ void k_emd_list_close(uint32_t* __restrict__ words, uint32_t cap, unsigned long long* __restrict__ totals, uint32_t* __restrict__ fold_flag, uint32_t n_blocks,
                                 uint32_t words_stride) {
	if (threadIdx.x || blockIdx.x) return;
	for (uint32_t j = 0; j < n_blocks; j++, words += words_stride) {
		if (fold_flag && words[1]) { totals[2] += 1; fold_flag[j] = 1; }
		else if (words[1]) totals[1] += 1;
		else totals[0] += words[0] < cap ? words[0] : cap;
		words[0] = 0;
		words[1] = 0;
	}
}

}  // namespace

// one wave per listed pair: four to a workgroup, at most num_cus * 8 workgroups. A group of blocks takes that many for its TOTAL capacity, shared out over
// blockIdx.y -- not a block's grid times the group
static dim3 list_grid(uint32_t cap, uint32_t n_blocks, int num_cus) {
	const uint64_t n = std::max<uint32_t>(n_blocks, 1), all = std::min<uint64_t>(n * (((uint64_t)cap + 3) / 4), (uint64_t)num_cus * 8);
	return dim3((unsigned)std::max<uint64_t>(1, (all + n - 1) / n), (unsigned)n);
}

// the two moments of slots [first_slot, first_slot + n_slots) from their 32-bit ranks
hipError_t msc_launch_rank_moments(hipStream_t st, uint64_t nbins, const uint32_t* ranks, uint64_t pitch, uint64_t first_slot, uint64_t n_slots, uint64_t* rk_sum, uint64_t* rk_dev) {
	if (n_slots == 0) return hipSuccess;
	k_rank_moments<<<dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, st>>>(ranks, pitch, nbins, first_slot, n_slots, rk_sum, rk_dev);
	return hipGetLastError();
}

// emd_list[i] = the distance of listed pair i, i < min(words[0], cap); two sets of one pitch. u16: both rows are the 16-bit form
hipError_t msc_launch_emd_ranks_list(hipStream_t st, bool u16, const void* c_ranks, const void* q_ranks, uint64_t pitch, const uint32_t* cand_slots, uint64_t first, uint32_t m_per_query,
                                     const uint32_t* q_slots_dev, const uint32_t* list, const uint32_t* words, uint32_t cap, uint64_t* emd_list, int num_cus,
                                     const MscListGroup* grp) {
	if (cap == 0) return hipSuccess;
	if (pitch % (u16 ? 1024 : 256) || m_per_query == 0) return hipErrorInvalidValue;
	const MscListGroup g = grp ? *grp : MscListGroup{1, 0, 0, 0, 0, 0, 0};
	const dim3 grid = list_grid(cap, g.n_blocks, num_cus);
	if (u16) k_emd_ranks_list<true><<<grid, dim3(256), 0, st>>>(c_ranks, q_ranks, pitch, cand_slots, first, m_per_query, q_slots_dev, list, words, cap, emd_list, g);
	else k_emd_ranks_list<false><<<grid, dim3(256), 0, st>>>(c_ranks, q_ranks, pitch, cand_slots, first, m_per_query, q_slots_dev, list, words, cap, emd_list, g);
	return hipGetLastError();
}

hipError_t msc_launch_fold_exact_list(hipStream_t st, const MscFoldExact& a, int num_cus, const MscListGroup* grp) {
	if (a.cap == 0) return hipSuccess;
	if (a.m_per_query == 0 || a.slices == 0 || a.slices > 64 || !a.c_ranks || !a.qT || !a.out_min) return hipErrorInvalidValue;
	const MscListGroup g = grp ? *grp : MscListGroup{1, 0, 0, 0, 0, 0, 0};
	k_fold_exact_list<<<list_grid(a.cap, g.n_blocks, num_cus), dim3(256), 0, st>>>(a, g);
	return hipGetLastError();
}

hipError_t msc_launch_emd_list_close(hipStream_t st, uint32_t* words, uint32_t cap, uint64_t* totals, uint32_t* fold_flag, uint32_t n_blocks, uint32_t words_stride) {
	k_emd_list_close<<<dim3(1), dim3(64), 0, st>>>(words, cap, (unsigned long long*)totals, fold_flag, n_blocks, words_stride);
	return hipGetLastError();
}
