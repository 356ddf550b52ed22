// msc_canonical.hip -- msc_hist_canonical_batch on the device: every k-mer counted together with its reverse complement,
//   canon(D)[b] = clamp(D[b] + D[msc_rc_bin(b)] - 1, 0, max(T))          (D holds the pseudocount of 1 in every bin; the sum is exact before the clamp)
// so that a sequence and its reverse complement become the same point. Each form mirrors one of msc_revcomp.hip, whose plan and index rule it shares.
//
//   dense   k_hist_canonical_lds : a slot of at most 64 KiB goes through LDS whole, one workgroup per slot (padding stays at the logical end)
//           k_hist_canonical     : larger slots by the tile transpose of k_hist_revcomp (msc_revcomp_plan.h). The free bits of a tile are closed under
//                                  the permutation (fs == fd), so the tiles of a slot fall into PAIRS that are each other's source: a work item takes
//                                  a tile and its partner, reads both into registers, turns each through LDS for the other and writes both. A tile is
//                                  read once per tile written, and nothing a work item writes is read by another: the in-place form is the same launch.
//           k_canonical_record   : length, id, overflow and n_kmers from the source, one_mers'[i] = one_mers[i] + one_mers[3 - i] - 1; the sums, the
//                                  magnitude, stddev and the tile prefixes come from msc_launch_finalize afterwards, as after msc_hist_upload
//   sparse  k_sparse_canonical_count : entries of the merged list (the source's own plus the mapped bins it does not hold)
//           k_sparse_canonical_sort  : lists of at most 16 384 entries, one workgroup per slot: source and mapped bins sorted together in LDS, equal
//                                      bins folded, values from the source list by bisection (a stored value includes the pseudocount, an absent bin
//                                      holds 1), cum, the sub-range table and the record's sums rebuilt (the slot k_sparse_build_sort writes)
//           longer lists: msc_launch_sparse_revcomp_scatter into a dense scratch slot, k_hist_canonical in place on it (canon(rc(D)) = canon(D)),
//                         then k_sparse_count / k_sparse_write (msc_api.hip)
// Saturation and the overflow flag are decided here, on the exact 64-bit sum (uint64_t bins: on the carry).
#include <algorithm>

#include "msc_internal.h"
#include "msc_revcomp_plan.h"
#include "msc_wave.h"

namespace {

constexpr int kCnBlock = 256;

// D[b] + D[rc(b)] - 1, clamped; *ovf is set when the exact sum is past max(T)
template <typename T>
__device__ __forceinline__ T canon_sum(T a, T b, uint32_t* ovf) {
	if constexpr (sizeof(T) == 8) {
		const uint64_t s = a + b;
		if (s < a) {          // carried: the exact value is 2^64 + s - 1
			if (s != 0) *ovf = 1;
			return ~0ull;
		}
		return s ? s - 1 : 0;
	} else {
		constexpr uint64_t tmax = (1ull << (8 * sizeof(T))) - 1;
		const uint64_t s = (uint64_t)a + (uint64_t)b;
		if (s == 0) return 0;
		if (s - 1 > tmax) { *ovf = 1; return (T)tmax; }
		return (T)(s - 1);
	}
}

__device__ __forceinline__ MscSlotScalars* cn_record(uint8_t* scalars, uint64_t stride, uint32_t slot) {
	return reinterpret_cast<MscSlotScalars*>(scalars + (uint64_t)slot * stride);
}

// (dst_bins and src_bins may be one array, and a pair may name one slot twice: the slot is in LDS before anything is written)
template <typename T>
__global__ void __launch_bounds__(kCnBlock) k_hist_canonical_lds(T* dst_bins, const T* src_bins, uint8_t* dst_scalars, uint64_t scalar_stride, const uint32_t* __restrict__ ds,
                                                                  const uint32_t* __restrict__ ss, uint64_t slot_elems, uint64_t nbins, int k, uint32_t R) {
	extern __shared__ __attribute__((aligned(16))) unsigned char cn_smem[];
	constexpr uint32_t E = 16 / sizeof(T);
	const T* tile = reinterpret_cast<const T*>(cn_smem);
	const uint32_t pair = blockIdx.x, chunks = (uint32_t)(slot_elems / E);
	const uint4* src = reinterpret_cast<const uint4*>(src_bins + (uint64_t)ss[pair] * slot_elems);
	uint4* dst = reinterpret_cast<uint4*>(dst_bins + (uint64_t)ds[pair] * slot_elems);
	for (uint32_t c = threadIdx.x; c < chunks; c += kCnBlock) reinterpret_cast<uint4*>(cn_smem)[c] = src[c];
	__syncthreads();
	uint32_t ovf = 0;
	for (uint32_t c = threadIdx.x; c < chunks; c += kCnBlock) {
		uint4 v;
		T* e = reinterpret_cast<T*>(&v);
#pragma unroll
		for (uint32_t j = 0; j < E; j++) {
			const uint64_t b = msc_logical_index((uint64_t)c * E + j, E, R);
			e[j] = b < nbins ? canon_sum<T>(tile[(uint64_t)c * E + j], tile[msc_phys_index(msc_rc_bin(b, k), E, R)], &ovf) : (T)0;
		}
		dst[c] = v;
	}
	if (ovf) cn_record(dst_scalars, scalar_stride, ds[pair])->overflow = 1;
}

// work item = (pair, tile of the slot); an item whose partner tile lies below it is the partner's. The per-thread offsets are k_hist_revcomp's, and
// with fs == fd the chunks of the partner tile sit at the same offsets from its base
template <typename T, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_hist_canonical(T* dst_bins, const T* src_bins, uint8_t* dst_scalars, uint64_t scalar_stride, const uint32_t* __restrict__ ds,
                                                          const uint32_t* __restrict__ ss, uint64_t slot_elems, MscRcPlan p, uint64_t n_items) {
	extern __shared__ __attribute__((aligned(16))) unsigned char cn_smem[];
	constexpr uint32_t E = 16 / sizeof(T);
	constexpr uint32_t lgE = E == 16 ? 4 : E == 8 ? 3 : E == 4 ? 2 : 1;
	constexpr uint32_t kMaxPer = MSC_RC_MAX_CHUNKS(T) / BLOCK;
	T* tile = reinterpret_cast<T*>(cn_smem);
	const uint32_t per = ((1u << p.f_bits) / E) / blockDim.x;
	const uint64_t z = msc_rc_phys(0, p.k, E, p.R);
	uint32_t off[kMaxPer], at_in[kMaxPer], at_out[kMaxPer], delta[E];
#pragma unroll
	for (uint32_t j = 0; j < E; j++) delta[j] = msc_rc_swizzle((uint32_t)msc_bits_extract(msc_rc_phys(j, p.k, E, p.R) ^ z, p.fd), p, lgE);
#pragma unroll
	for (uint32_t i = 0; i < kMaxPer; i++) {
		const uint32_t c = (threadIdx.x + i * blockDim.x) * E;
		off[i] = (uint32_t)msc_bits_deposit(c, p.fd);
		at_in[i] = msc_rc_swizzle((uint32_t)msc_bits_extract(msc_rc_phys((z & ~p.fd) | off[i], p.k, E, p.R), p.fd), p, lgE);
		at_out[i] = msc_rc_swizzle(c, p, lgE);
	}
	const uint32_t tiles_bits = p.n_bits - p.f_bits;
	const uint64_t all = (1ull << p.n_bits) - 1;
	for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
		const uint64_t pair = item >> tiles_bits, g = item & ((1ull << tiles_bits) - 1);
		const uint64_t a_base = msc_bits_deposit(g, all & ~p.fd);
		const uint64_t b_base = msc_rc_phys(a_base, p.k, E, p.R) & ~p.fd;
		if (b_base < a_base) continue;          // (the same for every thread of the workgroup)
		const bool two = b_base != a_base;
		const T* src = src_bins + (uint64_t)ss[pair] * slot_elems;
		T* dst = dst_bins + (uint64_t)ds[pair] * slot_elems;
		uint4 va[kMaxPer], vb[kMaxPer];
#pragma unroll
		for (uint32_t i = 0; i < kMaxPer; i++)
			if (i < per) {
				va[i] = *reinterpret_cast<const uint4*>(src + a_base + off[i]);
				vb[i] = two ? *reinterpret_cast<const uint4*>(src + b_base + off[i]) : va[i];
			}
		uint32_t ovf = 0;
#pragma unroll
		for (int half = 0; half < 2; half++) {
			if (half == 1 && !two) break;
			const uint4* own = half == 0 ? va : vb;          // the tile written in this half, and the one that is turned for it
			const uint4* other = half == 0 ? vb : va;
			__syncthreads();          // (the tile of the half before has been read out)
#pragma unroll
			for (uint32_t i = 0; i < kMaxPer; i++)
				if (i < per) {
					const T* e = reinterpret_cast<const T*>(&other[i]);
					uint32_t at = at_in[i];
					asm volatile("" : "+v"(at));
#pragma unroll
					for (uint32_t j = 0; j < E; j++) tile[at ^ delta[j]] = e[j];
				}
			__syncthreads();
#pragma unroll
			for (uint32_t i = 0; i < kMaxPer; i++)
				if (i < per) {          // (the sums go out through `turned`: half 1 still has to turn va as it was read)
					uint4 turned = *reinterpret_cast<const uint4*>(tile + at_out[i]);
					const T* x = reinterpret_cast<const T*>(&own[i]);
					T* y = reinterpret_cast<T*>(&turned);
#pragma unroll
					for (uint32_t j = 0; j < E; j++) y[j] = canon_sum<T>(x[j], y[j], &ovf);
					*reinterpret_cast<uint4*>(dst + (half == 0 ? a_base : b_base) + off[i]) = turned;
				}
		}
		if (ovf) cn_record(dst_scalars, scalar_stride, ds[pair])->overflow = 1;
	}
}

// one wave per pair, before the bins: the words of the record that do not follow from the bins
__global__ void __launch_bounds__(64) k_canonical_record(uint8_t* dst_scalars, const uint8_t* src_scalars, uint64_t scalar_stride, const uint32_t* __restrict__ ds,
                                                         const uint32_t* __restrict__ ss) {
	MscSlotScalars* to = cn_record(dst_scalars, scalar_stride, ds[blockIdx.x]);
	const MscSlotScalars* from = reinterpret_cast<const MscSlotScalars*>(src_scalars + (uint64_t)ss[blockIdx.x] * scalar_stride);
	const uint32_t lane = threadIdx.x;
	uint64_t a = 0, b = 0;
	if (lane < 4) { a = from->one_mers[lane]; b = from->one_mers[3 - lane]; }
	const uint64_t length = from->length, overflow = from->overflow, id = from->id, n_kmers = from->n_kmers;
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");          // (in place: every lane has read before any lane writes)
	__builtin_amdgcn_wave_barrier();
	if (lane < 4) to->one_mers[lane] = a + b - 1;
	if (lane == 4) { to->length = length; to->overflow = overflow; to->id = id; to->n_kmers = n_kmers; to->reserved[0] = to->reserved[1] = to->reserved[2] = 0; }
}

// ------------------------------------------------------------------------------------------------ sparse
__device__ __forceinline__ uint32_t cn_lookup(const uint2* __restrict__ src, uint32_t n, uint32_t bin) {          // the value of a bin: the pseudocount where it is not stored
	uint32_t lo = 0, hi = n;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (src[mid].x < bin) lo = mid + 1; else hi = mid; }
	return lo < n && src[lo].x == bin ? src[lo].y : 1u;
}

__device__ __forceinline__ uint64_t cn_wave_sum(uint64_t v) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

__global__ void __launch_bounds__(kCnBlock) k_sparse_canonical_count(int k, const uint2* __restrict__ s_ent, const MscSparseHdr* __restrict__ s_hdr, const uint32_t* __restrict__ ss,
                                                                      uint32_t* __restrict__ counts) {
	extern __shared__ __attribute__((aligned(16))) unsigned char cn_smem[];
	uint64_t* s_part = reinterpret_cast<uint64_t*>(cn_smem);
	const MscSparseHdr sh = s_hdr[ss[blockIdx.x]];
	const uint2* src = s_ent + sh.off;
	uint64_t extra = 0;
	for (uint32_t i = threadIdx.x; i < sh.nnz; i += kCnBlock) {
		const uint32_t r = (uint32_t)msc_rc_bin(src[i].x, k);
		uint32_t lo = 0, hi = sh.nnz;
		while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (src[mid].x < r) lo = mid + 1; else hi = mid; }
		if (!(lo < sh.nnz && src[lo].x == r)) extra++;
	}
	extra = cn_wave_sum(extra);
	if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = extra;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t t = sh.nnz;
		for (int i = 0; i < kCnBlock / 64; i++) t += s_part[i];
		counts[blockIdx.x] = (uint32_t)t;
	}
}

// One workgroup per pair (k_sparse_build_sort's plan): the keys are the source's bins and their images, sorted in LDS; a run of equal keys (a bin and
// its partner both stored; a palindrome) is one entry. (s_hdr and d_hdr may be one array: the source's header is read before anything is written.)
__global__ void __launch_bounds__(kCnBlock) k_sparse_canonical_sort(int k, int dtype, uint64_t nbins, const uint2* __restrict__ s_ent, const MscSparseHdr* s_hdr,
                                                                     const uint32_t* __restrict__ ds, const uint32_t* __restrict__ ss, const uint64_t* __restrict__ dst_off,
                                                                     uint32_t P /* power of two >= twice the longest list of the launch, >= kCnBlock */, uint2* __restrict__ d_ent,
                                                                     uint32_t* __restrict__ d_cum, MscSparseHdr* d_hdr, MscSparseHdr* __restrict__ hdr_list, uint8_t* dst_scalars,
                                                                     uint64_t scalar_stride) {
	extern __shared__ __attribute__((aligned(16))) unsigned char cn_smem[];
	uint32_t* keys = reinterpret_cast<uint32_t*>(cn_smem);          // P keys | a head count per thread | the sub-range table (32 words) | 64-bit: an excess per thread, 4 x 4 partial reductions
	uint32_t* s_cnt = keys + P;
	uint32_t* s_split = s_cnt + kCnBlock;
	uint64_t* s_ex = reinterpret_cast<uint64_t*>(s_split + 32);
	uint64_t* s_red = s_ex + kCnBlock;
	const uint32_t pair = blockIdx.x, tid = threadIdx.x;
	const MscSparseHdr sh = s_hdr[ss[pair]];
	const uint32_t n = sh.nnz, n2 = 2 * n;
	if (n2 > P) return;          // (longer lists are not this kernel's: the host sends them to the scratch route)
	const uint2* src = s_ent + sh.off;
	for (uint32_t i = tid; i < P; i += kCnBlock) keys[i] = i < n ? src[i].x : i < n2 ? (uint32_t)msc_rc_bin(src[i - n].x, k) : 0xffffffffu;
	__syncthreads();
	for (uint32_t size = 2; size <= P; size <<= 1) {
		for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
			for (uint32_t t = tid; t < P / 2; t += kCnBlock) {
				const uint32_t lo = 2 * t - (t & (stride - 1));
				const uint32_t hi = lo + stride;
				const bool up = (lo & size) == 0;
				const uint32_t a = keys[lo], b = keys[hi];
				if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
			}
			__syncthreads();
		}
	}
	// thread t owns the keys [t * C, (t + 1) * C) of the sorted array
	const uint64_t tmax = dtype >= 32 ? 0xffffffffull : ((1ull << dtype) - 1);          // (an entry's value is 32 bits wide)
	const uint32_t C = P / kCnBlock;
	const uint32_t c0 = tid * C < n2 ? tid * C : n2, c1 = c0 + C < n2 ? c0 + C : n2;
	auto value = [&](uint32_t key, uint64_t* ovf) -> uint64_t {
		uint64_t v = (uint64_t)cn_lookup(src, n, key) + cn_lookup(src, n, (uint32_t)msc_rc_bin(key, k)) - 1;
		if (v > tmax) { v = tmax; *ovf = 1; }
		return v;
	};
	uint64_t cnt = 0, ex = 0, sq = 0, mx = 0, ovf = 0;
	for (uint32_t i = c0; i < c1; i++)
		if (i == 0 || keys[i] != keys[i - 1]) {
			const uint64_t v = value(keys[i], &ovf);
			cnt++; ex += v - 1; sq += v * v - 1; mx = v > mx ? v : mx;
		}
	s_cnt[tid] = (uint32_t)cnt;
	s_ex[tid] = ex;
	__syncthreads();
	if (tid == 0) {          // 256-element exclusive scans: serial is fine
		uint32_t a = 0;
		uint64_t b = 0;
		for (int i = 0; i < kCnBlock; i++) { const uint32_t x = s_cnt[i]; const uint64_t y = s_ex[i]; s_cnt[i] = a; s_ex[i] = b; a += x; b += y; }
		s_red[0] = a;          // entries
		s_red[1] = b;          // total excess
	}
	__syncthreads();
	const uint64_t arena = dst_off[pair];
	{
		uint64_t o = arena + s_cnt[tid], unused = 0;
		uint32_t run = (uint32_t)s_ex[tid];
		for (uint32_t i = c0; i < c1; i++)
			if (i == 0 || keys[i] != keys[i - 1]) {
				const uint64_t v = value(keys[i], &unused);
				run += (uint32_t)(v - 1);
				d_ent[o] = make_uint2(keys[i], (uint32_t)v);
				d_cum[o] = run;
				o++;
			}
	}
	if (tid <= MSC_SPARSE_SUB) {          // entries with a bin under w * 4^k / 16 == run heads before the first key at or past that bound
		const uint64_t bound = nbins / MSC_SPARSE_SUB * tid;
		uint32_t lo = 0, hi = n2;
		while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)keys[mid] < bound) lo = mid + 1; else hi = mid; }
		const uint32_t owner = lo / C < (uint32_t)kCnBlock ? lo / C : kCnBlock - 1;
		uint32_t heads = s_cnt[owner];
		for (uint32_t i = owner * C; i < lo; i++) if (i == 0 || keys[i] != keys[i - 1]) heads++;
		s_split[tid] = tid == MSC_SPARSE_SUB ? (uint32_t)s_red[0] : heads;
	}
	// the record's sums, from the entries (k_sparse_build_sort's; the expression for stddev is k_finalize's)
	sq = cn_wave_sum(sq);
	uint64_t m2 = mx, o2 = ovf;
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) { const uint64_t a = __shfl_xor(m2, off, 64); m2 = a > m2 ? a : m2; o2 |= __shfl_xor(o2, off, 64); }
	if ((tid & 63) == 0) { s_red[4 + (tid >> 6)] = sq; s_red[8 + (tid >> 6)] = m2; s_red[12 + (tid >> 6)] = o2; }
	__syncthreads();
	if (tid == 0) {
		uint64_t sqt = 0, mxt = 1, ov = 0;
		for (int i = 0; i < kCnBlock / 64; i++) { sqt += s_red[4 + i]; mxt = s_red[8 + i] > mxt ? s_red[8 + i] : mxt; ov |= s_red[12 + i]; }
		MscSlotScalars* sc = cn_record(dst_scalars, scalar_stride, ds[pair]);
		const uint64_t sum = nbins + s_red[1], sum_sq = nbins + sqt;
		sc->sum = sum; sc->sum_sq = sum_sq; sc->max_count = mxt; sc->mag = sum;
		if (ov) sc->overflow = 1;          // (k_canonical_record has copied the source's flag)
		const double N = (double)nbins, aq = (double)sum / N;
		const double var = ((double)sum_sq - 2.0 * aq * (double)sum + N * aq * aq) / N;
		sc->stddev = sqrt(var > 0 ? var : 0);
		MscSparseHdr h;
		h.off = arena;
		h.nnz = (uint32_t)s_red[0];
		for (int w = 0; w <= MSC_SPARSE_SUB; w++) h.split[w] = s_split[w];
		h.pad_[0] = h.pad_[1] = 0;
		d_hdr[ds[pair]] = h;
		hdr_list[pair] = h;
	}
}

}  // namespace

hipError_t msc_launch_canonical_record(hipStream_t st, uint8_t* dst_scalars, const uint8_t* src_scalars, uint64_t stride, const uint32_t* dst_slots, const uint32_t* src_slots,
                                       uint32_t n) {
	if (n == 0) return hipSuccess;
	k_canonical_record<<<dim3(n), dim3(64), 0, st>>>(dst_scalars, src_scalars, stride, dst_slots, src_slots);
	return hipGetLastError();
}

hipError_t msc_launch_hist_canonical(hipStream_t st, const MscLayout& L, int k, int dtype, uint8_t* dst_bins, uint8_t* dst_scalars, const uint8_t* src_bins,
                                     const uint8_t* src_scalars, const uint32_t* dst_slots, const uint32_t* src_slots, uint32_t n) {
	if (n == 0) return hipSuccess;
	const uint64_t stride = msc_scalar_stride(L.S);
	hipError_t e = msc_launch_canonical_record(st, dst_scalars, src_scalars, stride, dst_slots, src_slots, n);
	if (e != hipSuccess) return e;
	return msc_by_dtype(dtype, [&](auto tag) -> hipError_t {
		using T = decltype(tag);
		if (msc_revcomp_whole_slot(L)) {
			const size_t lds = (size_t)L.slot_bytes;
			if (lds > 48 * 1024) e = hipFuncSetAttribute((const void*)k_hist_canonical_lds<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
			if (e != hipSuccess) return e;
			k_hist_canonical_lds<T><<<dim3(n), dim3(kCnBlock), lds, st>>>((T*)dst_bins, (const T*)src_bins, dst_scalars, stride, dst_slots, src_slots, L.padded_bins, L.nbins, k, L.R);
		} else {
			if (L.nbins != L.padded_bins) return hipErrorInvalidValue;
			const MscRcPlan p = msc_rc_plan(L, k);
			const size_t lds = (size_t)L.esz << p.f_bits;
			constexpr int kBlockT = MSC_RC_MAX_CHUNKS(T) / 4 > 256 ? MSC_RC_MAX_CHUNKS(T) / 4 : 256;
			if (!msc_rc_plan_fits(p, L) || p.fs != p.fd) return hipErrorInvalidValue;          // (fs == fd: the permutation of the index bits is an involution)
			const uint32_t threads = std::min<uint32_t>(kBlockT, (1u << p.f_bits) / L.E);
			if (lds > 48 * 1024) e = hipFuncSetAttribute((const void*)k_hist_canonical<T, kBlockT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
			if (e != hipSuccess) return e;
			const uint64_t items = (uint64_t)n << (p.n_bits - p.f_bits);
			// an odd grid: the tiles of a slot are a power of two, so a workgroup's stride then meets every tile, the skipped halves of the pairs included, and the
			// work spreads evenly; many more workgroups than the device holds at once keep the last round short
			k_hist_canonical<T, kBlockT><<<dim3((unsigned)std::min<uint64_t>(items, 16383)), dim3(threads), lds, st>>>((T*)dst_bins, (const T*)src_bins, dst_scalars, stride, dst_slots,
			                                                                                                        src_slots, L.padded_bins, p, items);
		}
		return hipGetLastError();
	});
}

uint32_t msc_sparse_canonical_sort_max() { return 16384; }

hipError_t msc_launch_sparse_canonical_count(hipStream_t st, int k, const void* s_ent, const MscSparseHdr* s_hdr, const uint32_t* src_slots, uint32_t n, uint32_t* counts) {
	if (n == 0) return hipSuccess;
	k_sparse_canonical_count<<<dim3(n), dim3(kCnBlock), (kCnBlock / 64) * sizeof(uint64_t), st>>>(k, (const uint2*)s_ent, s_hdr, src_slots, counts);
	return hipGetLastError();
}

hipError_t msc_launch_sparse_canonical_sort(hipStream_t st, int k, int dtype, uint64_t nbins, const void* s_ent, const MscSparseHdr* s_hdr, const uint32_t* dst_slots,
                                            const uint32_t* src_slots, const uint64_t* dst_off, uint32_t n, uint32_t longest, void* d_ent, uint32_t* d_cum, MscSparseHdr* d_hdr,
                                            MscSparseHdr* hdr_list, uint8_t* dst_scalars, uint64_t scalar_stride) {
	if (n == 0) return hipSuccess;
	if (longest > msc_sparse_canonical_sort_max()) return hipErrorInvalidValue;
	uint32_t P = kCnBlock;
	while (P < 2 * longest) P <<= 1;
	auto lds_for = [](size_t keys) { return (keys + kCnBlock + 32) * sizeof(uint32_t) + (kCnBlock + 16) * sizeof(uint64_t); };
	static bool raised = false;
	if (!raised) {
		const hipError_t e = hipFuncSetAttribute((const void*)k_sparse_canonical_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_for(32768));
		if (e != hipSuccess) return e;
		raised = true;
	}
	k_sparse_canonical_sort<<<dim3(n), dim3(kCnBlock), lds_for(P), st>>>(k, dtype, nbins, (const uint2*)s_ent, s_hdr, dst_slots, src_slots, dst_off, P, (uint2*)d_ent, d_cum, d_hdr,
	                                                                      hdr_list, dst_scalars, scalar_stride);
	return hipGetLastError();
}
