// msc_revcomp.hip -- msc_hist_revcomp_batch on the device: the histogram of the reverse complement of whatever a slot counts is a fixed
// permutation of its bins, bins'[b] = bins[msc_rc_bin(b)] (msc_revcomp.h), so it exists for slots that have no sequence (centres, means).
//
//   dense   k_hist_revcomp_lds : a slot of at most 64 KiB goes through LDS whole, one workgroup per slot (padding stays at the logical end)
//           k_hist_revcomp     : larger slots as a digit-reversal transpose in tiles (msc_revcomp_plan.h): runs of 256 bytes read, the tile
//                                turned in LDS, runs of 256 bytes written as 16-byte stores in the tile-permuted order of msc_layout.h
//           k_revcomp_tile_sums + k_revcomp_record : the tile prefixes of the new bins (k_prefix's scan over a slot list) and the 1-mers reversed
//   sparse  k_sparse_revcomp_sort    : lists of at most 32 768 entries, one workgroup per slot: bins mapped, sorted in LDS, values looked up in the
//                                      source list, cum and the sub-range table rebuilt (the slot k_sparse_build_sort writes)
//           k_sparse_revcomp_scatter : longer lists into a dense scratch slot, which k_sparse_count / k_sparse_write compact (the builder's route)
#include <algorithm>

#include "msc_internal.h"
#include "msc_revcomp_plan.h"
#include "msc_wave.h"

namespace {

constexpr int kRcBlock = 256;

template <typename T>
__global__ void __launch_bounds__(kRcBlock) k_hist_revcomp_lds(T* __restrict__ dst_bins, const T* __restrict__ src_bins, const uint32_t* __restrict__ ds,
                                                                const uint32_t* __restrict__ ss, uint64_t slot_elems, uint64_t nbins, int k, uint32_t R) {
	extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
	constexpr uint32_t E = 16 / sizeof(T);
	T* tile = reinterpret_cast<T*>(rc_smem);
	const uint32_t pair = blockIdx.x, chunks = (uint32_t)(slot_elems / E);
	const uint4* src = reinterpret_cast<const uint4*>(src_bins + (uint64_t)ss[pair] * slot_elems);
	uint4* dst = reinterpret_cast<uint4*>(dst_bins + (uint64_t)ds[pair] * slot_elems);
	for (uint32_t c = threadIdx.x; c < chunks; c += kRcBlock) reinterpret_cast<uint4*>(rc_smem)[c] = src[c];
	__syncthreads();
	for (uint32_t c = threadIdx.x; c < chunks; c += kRcBlock) {
		uint4 v;
		T* e = reinterpret_cast<T*>(&v);
#pragma unroll
		for (uint32_t j = 0; j < E; j++) {
			const uint64_t b = msc_logical_index((uint64_t)c * E + j, E, R);
			e[j] = b < nbins ? tile[msc_phys_index(msc_rc_bin(b, k), E, R)] : (T)0;
		}
		dst[c] = v;
	}
}

// work item = (pair, tile of the slot); the workgroups stride over them. What a thread's chunks read, where their elements go in LDS and what they
// write is the same for every tile (the map is affine: a tile's fixed bits only move its base), so it is worked out once, into registers
template <typename T, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_hist_revcomp(T* __restrict__ dst_bins, const T* __restrict__ src_bins, const uint32_t* __restrict__ ds,
                                                            const uint32_t* __restrict__ ss, uint64_t slot_elems, MscRcPlan p, uint64_t n_items) {
	extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
	constexpr uint32_t E = 16 / sizeof(T);
	constexpr uint32_t lgE = E == 16 ? 4 : E == 8 ? 3 : E == 4 ? 2 : 1;
	constexpr uint32_t kMaxPer = MSC_RC_MAX_CHUNKS(T) / BLOCK;          // 16-byte chunks of a tile per thread, at most (4; u64: 2)
	T* tile = reinterpret_cast<T*>(rc_smem);
	const uint32_t per = ((1u << p.f_bits) / E) / blockDim.x;          // (the launch has min(BLOCK, chunks of a tile) threads)
	const uint64_t z = msc_rc_phys(0, p.k, E, p.R);
	uint32_t s_off[kMaxPer], at_in[kMaxPer], d_off[kMaxPer], at_out[kMaxPer], delta[E];
#pragma unroll
	for (uint32_t j = 0; j < E; j++) delta[j] = msc_rc_swizzle((uint32_t)msc_bits_extract(msc_rc_phys(j, p.k, E, p.R) ^ z, p.fd), p, lgE);
#pragma unroll
	for (uint32_t i = 0; i < kMaxPer; i++) {
		const uint32_t c = (threadIdx.x + i * blockDim.x) * E;
		s_off[i] = (uint32_t)msc_bits_deposit(c, p.fs);
		at_in[i] = msc_rc_swizzle((uint32_t)msc_bits_extract(msc_rc_phys((z & ~p.fs) | s_off[i], p.k, E, p.R), p.fd), p, lgE);
		d_off[i] = (uint32_t)msc_bits_deposit(c, p.fd);
		at_out[i] = msc_rc_swizzle(c, p, lgE);
	}
	const uint32_t tiles_bits = p.n_bits - p.f_bits;
	const uint64_t all = (1ull << p.n_bits) - 1;
	for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
		const uint64_t pair = item >> tiles_bits, g = item & ((1ull << tiles_bits) - 1);
		const uint64_t d_base = msc_bits_deposit(g, all & ~p.fd);
		const uint64_t s_base = msc_rc_phys(d_base, p.k, E, p.R) & ~p.fs;
		const T* src = src_bins + (uint64_t)ss[pair] * slot_elems + s_base;
		T* dst = dst_bins + (uint64_t)ds[pair] * slot_elems + d_base;
		uint4 v[kMaxPer];
#pragma unroll
		for (uint32_t i = 0; i < kMaxPer; i++)
			if (i < per) v[i] = *reinterpret_cast<const uint4*>(src + s_off[i]);
		__syncthreads();          // (the tile of the item before has been written out)
#pragma unroll
		for (uint32_t i = 0; i < kMaxPer; i++)
			if (i < per) {
				const T* e = reinterpret_cast<const T*>(&v[i]);
				uint32_t at = at_in[i];
				asm volatile("" : "+v"(at));          // (keeps the 4 x E sums at ^ delta[j] out of registers that live across the items: one XOR each)
#pragma unroll
				for (uint32_t j = 0; j < E; j++) tile[at ^ delta[j]] = e[j];
			}
		__syncthreads();
#pragma unroll
		for (uint32_t i = 0; i < kMaxPer; i++)
			if (i < per) *reinterpret_cast<uint4*>(dst + d_off[i]) = *reinterpret_cast<const uint4*>(tile + at_out[i]);
	}
}

__device__ __forceinline__ uint64_t rc_wave_sum(uint64_t v) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

// one wave per (pair, tile): the tile's sum into the record's tile array (k_finalize's, for a slot list)
template <typename T>
__global__ void __launch_bounds__(kRcBlock) k_revcomp_tile_sums(const T* __restrict__ bins, uint8_t* __restrict__ scalars, uint64_t scalar_stride, uint64_t slot_elems,
                                                                 const uint32_t* __restrict__ ds, uint64_t n, uint32_t S, uint32_t tile_bins) {
	constexpr uint32_t E = 16 / sizeof(T);
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t W = (uint64_t)blockIdx.x * (kRcBlock / 64) + (threadIdx.x >> 6);
	if (W >= n * S) return;
	const uint64_t slot = ds[W / S];
	const uint32_t t = (uint32_t)(W % S);
	const T* h = bins + slot * slot_elems + (uint64_t)t * tile_bins;
	uint64_t ts = 0;
	for (uint32_t l = 0; l < tile_bins / (64 * E); l++) {
		const uint4 v = *reinterpret_cast<const uint4*>(h + (uint64_t)l * 64 * E + lane * E);
		const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
		for (uint32_t j = 0; j < E; j++) ts += e[j];
	}
	ts = rc_wave_sum(ts);
	if (lane == 0) reinterpret_cast<uint64_t*>(scalars + slot * scalar_stride + sizeof(MscSlotScalars))[t] = ts;
}

// one wave per pair: the tile sums scanned into exclusive prefixes (k_prefix; S = 0: a sparse slot has none), the 1-mers of the source reversed
__global__ void __launch_bounds__(64) k_revcomp_record(uint8_t* __restrict__ dst_scalars, const uint8_t* __restrict__ src_scalars, uint64_t scalar_stride,
                                                       const uint32_t* __restrict__ ds, const uint32_t* __restrict__ ss, uint32_t S) {
	uint8_t* rec = dst_scalars + (uint64_t)ds[blockIdx.x] * scalar_stride;
	const MscSlotScalars* from = reinterpret_cast<const MscSlotScalars*>(src_scalars + (uint64_t)ss[blockIdx.x] * scalar_stride);
	uint64_t* p = reinterpret_cast<uint64_t*>(rec + sizeof(MscSlotScalars));
	const uint32_t lane = threadIdx.x;
	if (lane < 4) reinterpret_cast<MscSlotScalars*>(rec)->one_mers[lane] = from->one_mers[3 - lane];
	uint64_t carry = 0;
	for (uint32_t base = 0; base < S; base += 64) {
		const uint32_t i = base + lane;
		const uint64_t v = i < S ? p[i] : 0;
		uint64_t inc = v;
#pragma unroll
		for (int off = 1; off < 64; off <<= 1) {
			const uint64_t o = __shfl_up(inc, off, 64);
			if ((int)lane >= off) inc += o;
		}
		if (i < S) p[i] = carry + inc - v;
		carry += __shfl(inc, 63, 64);
	}
}

// ------------------------------------------------------------------------------------------------ sparse
// One workgroup per pair (k_sparse_build_sort's plan): the mapped bins are the keys, sorted in LDS; a bin is stored once, so the sorted position
// of a key is its entry, and its value is that of msc_rc_bin(key) in the source list, found by bisection.
__global__ void __launch_bounds__(kRcBlock) k_sparse_revcomp_sort(int k, uint64_t nbins, const uint2* __restrict__ s_ent, const MscSparseHdr* __restrict__ s_hdr,
                                                                   const uint32_t* __restrict__ ds, const uint32_t* __restrict__ ss, const uint64_t* __restrict__ dst_off,
                                                                   uint32_t P /* power of two >= the longest list of the launch, >= kRcBlock */, uint2* __restrict__ d_ent,
                                                                   uint32_t* __restrict__ d_cum, MscSparseHdr* __restrict__ d_hdr, MscSparseHdr* __restrict__ hdr_list /* the same headers in launch order, for the host */) {
	extern __shared__ __attribute__((aligned(16))) unsigned char rc_smem[];
	uint32_t* keys = reinterpret_cast<uint32_t*>(rc_smem);          // P keys, then one excess sum per thread, then the sub-range table
	uint32_t* s_ex = keys + P;
	uint32_t* s_split = s_ex + kRcBlock;
	const uint32_t pair = blockIdx.x, tid = threadIdx.x;
	const MscSparseHdr sh = s_hdr[ss[pair]];
	const uint32_t n = sh.nnz;
	if (n > P) return;          // (longer lists are not this kernel's: the host sends them to the scratch route)
	const uint2* src = s_ent + sh.off;
	for (uint32_t i = tid; i < P; i += kRcBlock) keys[i] = i < n ? (uint32_t)msc_rc_bin(src[i].x, k) : 0xffffffffu;
	__syncthreads();
	for (uint32_t size = 2; size <= P; size <<= 1) {
		for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
			for (uint32_t t = tid; t < P / 2; t += kRcBlock) {
				const uint32_t lo = 2 * t - (t & (stride - 1));
				const uint32_t hi = lo + stride;
				const bool up = (lo & size) == 0;
				const uint32_t a = keys[lo], b = keys[hi];
				if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
			}
			__syncthreads();
		}
	}
	// thread t owns the entries [t * C, (t + 1) * C) of the sorted list
	const uint32_t C = P / kRcBlock;
	const uint32_t c0 = tid * C < n ? tid * C : n, c1 = c0 + C < n ? c0 + C : n;
	const uint64_t o = dst_off[pair];
	uint32_t ex = 0;
	for (uint32_t i = c0; i < c1; i++) {
		const uint32_t key = keys[i], old = (uint32_t)msc_rc_bin(key, k);
		uint32_t lo = 0, hi = n;
		while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (src[mid].x < old) lo = mid + 1; else hi = mid; }
		const uint32_t v = src[lo < n ? lo : n - 1].y;
		d_ent[o + i] = make_uint2(key, v);
		ex += v - 1;
	}
	s_ex[tid] = ex;
	__syncthreads();
	if (tid == 0) {          // 256-element exclusive scan: serial is fine
		uint32_t a = 0;
		for (int i = 0; i < kRcBlock; i++) { const uint32_t x = s_ex[i]; s_ex[i] = a; a += x; }
	}
	if (tid <= MSC_SPARSE_SUB) {          // entries with a bin under w * 4^k / 16
		const uint64_t bound = nbins / MSC_SPARSE_SUB * tid;
		uint32_t lo = 0, hi = n;
		while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)keys[mid] < bound) lo = mid + 1; else hi = mid; }
		s_split[tid] = tid == MSC_SPARSE_SUB ? n : lo;
	}
	__syncthreads();
	uint32_t run = s_ex[tid];
	for (uint32_t i = c0; i < c1; i++) {
		run += d_ent[o + i].y - 1;          // (this thread's own store above)
		d_cum[o + i] = run;
	}
	if (tid == 0) {
		MscSparseHdr h;
		h.off = o;
		h.nnz = n;
		for (int w = 0; w <= MSC_SPARSE_SUB; w++) h.split[w] = s_split[w];
		h.pad_[0] = h.pad_[1] = 0;
		d_hdr[ds[pair]] = h;
		hdr_list[pair] = h;
	}
}

// the entries of one list into a dense slot that holds the pseudocount everywhere
template <typename T>
__global__ void __launch_bounds__(kRcBlock) k_sparse_revcomp_scatter(T* __restrict__ bins, const uint2* __restrict__ ent, uint32_t n, int k, uint32_t R) {
	constexpr uint32_t E = 16 / sizeof(T);
	for (uint64_t i = (uint64_t)blockIdx.x * kRcBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kRcBlock) {
		const uint2 e = ent[i];
		bins[msc_phys_index(msc_rc_bin(e.x, k), E, R)] = (T)e.y;
	}
}

}  // namespace

bool msc_revcomp_whole_slot(const MscLayout& L) { return L.slot_bytes <= 64 * 1024; }

hipError_t msc_launch_hist_revcomp(hipStream_t st, const MscLayout& L, int k, int dtype, uint8_t* dst_bins, uint8_t* dst_scalars, const uint8_t* src_bins,
                                   const uint8_t* src_scalars, const uint32_t* dst_slots, const uint32_t* src_slots, uint32_t n) {
	if (n == 0) return hipSuccess;
	const uint64_t stride = msc_scalar_stride(L.S);
	return msc_by_dtype(dtype, [&](auto tag) -> hipError_t {
		using T = decltype(tag);
		hipError_t e = hipSuccess;
		if (msc_revcomp_whole_slot(L)) {
			const size_t lds = (size_t)L.slot_bytes;
			if (lds > 48 * 1024) e = hipFuncSetAttribute((const void*)k_hist_revcomp_lds<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
			if (e != hipSuccess) return e;
			k_hist_revcomp_lds<T><<<dim3(n), dim3(kRcBlock), lds, st>>>((T*)dst_bins, (const T*)src_bins, dst_slots, src_slots, L.padded_bins, L.nbins, k, L.R);
		} else {
			if (L.nbins != L.padded_bins) return hipErrorInvalidValue;
			const MscRcPlan p = msc_rc_plan(L, k);
			const size_t lds = (size_t)L.esz << p.f_bits;
			// a workgroup per tile with four 16-byte chunks a thread where the tile has them: 1 024 threads for 64 KiB of uint8_t, 256 for 16 KiB of uint32_t
			constexpr int kBlockT = MSC_RC_MAX_CHUNKS(T) / 4 > 256 ? MSC_RC_MAX_CHUNKS(T) / 4 : 256;
			if (!msc_rc_plan_fits(p, L)) return hipErrorInvalidValue;
			const uint32_t threads = std::min<uint32_t>(kBlockT, (1u << p.f_bits) / L.E);
			if (lds > 48 * 1024) e = hipFuncSetAttribute((const void*)k_hist_revcomp<T, kBlockT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
			if (e != hipSuccess) return e;
			const uint64_t items = (uint64_t)n << (p.n_bits - p.f_bits);
			k_hist_revcomp<T, kBlockT><<<dim3((unsigned)std::min<uint64_t>(items, 4096)), dim3(threads), lds, st>>>((T*)dst_bins, (const T*)src_bins, dst_slots, src_slots,
			                                                                                                  L.padded_bins, p, items);
		}
		if ((e = hipGetLastError()) != hipSuccess) return e;
		const uint64_t waves = (uint64_t)n * L.S;
		k_revcomp_tile_sums<T><<<dim3((unsigned)((waves + kRcBlock / 64 - 1) / (kRcBlock / 64))), dim3(kRcBlock), 0, st>>>((const T*)dst_bins, dst_scalars, stride, L.padded_bins,
		                                                                                                                 dst_slots, n, L.S, L.tile_bins);
		if ((e = hipGetLastError()) != hipSuccess) return e;
		k_revcomp_record<<<dim3(n), dim3(64), 0, st>>>(dst_scalars, src_scalars, stride, dst_slots, src_slots, L.S);
		return hipGetLastError();
	});
}

hipError_t msc_launch_revcomp_one_mers(hipStream_t st, uint8_t* dst_scalars, const uint8_t* src_scalars, uint64_t stride, const uint32_t* dst_slots,
                                       const uint32_t* src_slots, uint32_t n) {
	if (n == 0) return hipSuccess;
	k_revcomp_record<<<dim3(n), dim3(64), 0, st>>>(dst_scalars, src_scalars, stride, dst_slots, src_slots, 0);
	return hipGetLastError();
}

uint32_t msc_sparse_revcomp_sort_max() { return 32768; }

hipError_t msc_launch_sparse_revcomp_sort(hipStream_t st, int k, uint64_t nbins, const void* s_ent, const MscSparseHdr* s_hdr, const uint32_t* dst_slots,
                                          const uint32_t* src_slots, const uint64_t* dst_off, uint32_t n, uint32_t longest, void* d_ent, uint32_t* d_cum, MscSparseHdr* d_hdr,
                                          MscSparseHdr* hdr_list) {
	if (n == 0) return hipSuccess;
	if (longest > msc_sparse_revcomp_sort_max()) return hipErrorInvalidValue;
	uint32_t P = kRcBlock;
	while (P < longest) P <<= 1;
	const size_t lds = ((size_t)P + kRcBlock + 32) * sizeof(uint32_t);
	static bool raised = false;
	if (!raised) {
		const hipError_t e = hipFuncSetAttribute((const void*)k_sparse_revcomp_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (32768 + kRcBlock + 32) * 4);
		if (e != hipSuccess) return e;
		raised = true;
	}
	k_sparse_revcomp_sort<<<dim3(n), dim3(kRcBlock), lds, st>>>(k, nbins, (const uint2*)s_ent, s_hdr, dst_slots, src_slots, dst_off, P, (uint2*)d_ent, d_cum, d_hdr, hdr_list);
	return hipGetLastError();
}

hipError_t msc_launch_sparse_revcomp_scatter(hipStream_t st, const MscLayout& L, int k, int dtype, void* scratch_bins, const void* ent, uint32_t n) {
	if (n == 0) return hipSuccess;
	return msc_by_dtype(dtype, [&](auto tag) -> hipError_t {
		using T = decltype(tag);
		k_sparse_revcomp_scatter<T><<<dim3((n + kRcBlock - 1) / kRcBlock), dim3(kRcBlock), 0, st>>>((T*)scratch_bins, (const uint2*)ent, n, k, L.R);
		return hipGetLastError();
	});
}
