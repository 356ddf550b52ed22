// msc_revcomp_plan.h -- how k_hist_revcomp (msc_revcomp.hip) cuts the reverse-complement permutation of a dense slot into tiles.
//
// For a histogram of whole tiles the map  p -> msc_phys_index(msc_rc_bin(msc_logical_index(p)))  between the PHYSICAL element indices of the
// source and of the destination slot moves every index bit to another place and complements it: the tile permutation of msc_layout.h
// rearranges bit fields, the reverse complement reverses the bit pairs. It is its own inverse, and it is affine over the bits:
// rc_phys(a ^ b) = rc_phys(a) ^ rc_phys(b) ^ rc_phys(0). A digit-reversal transpose, so it is done as one: a workgroup owns the elements whose
// destination index varies in the bits of `fd` only -- the low `w` bits (a run of consecutive destination elements) and the bits whose images
// are the low `w` bits of the source index (a run of consecutive source elements) -- reads the source in whole runs, turns the tile in LDS
// and writes the destination in whole runs. Cut by bits, not by digits: a uint64_t tile is 2^9 bins.
#pragma once
#include "msc_revcomp.h"

struct MscRcPlan {
	int32_t k;
	uint32_t E, R;
	uint32_t n_bits;       // index bits of a slot (2k)
	uint32_t w;            // a run: 2^w elements (256 bytes)
	uint32_t f_bits;       // a tile: 2^f_bits elements, f_bits <= 2w
	uint64_t fd, fs;       // the free bits of a tile in the destination's / the source's physical index (fs = the image of fd)
	uint32_t swz_shift, swz_mask;      // LDS swizzle: the 16-byte chunk of a row ^= (row >> swz_shift) & swz_mask
};

MSC_HD uint64_t msc_rc_phys(uint64_t p, int k, uint32_t E, uint32_t R) { return msc_phys_index(msc_rc_bin(msc_logical_index(p, E, R), k), E, R); }

// the low bits of x spread over the set bits of mask, lowest first / the bits of x under mask gathered, lowest first
MSC_HD uint64_t msc_bits_deposit(uint64_t x, uint64_t mask) {
	uint64_t r = 0;
	while (mask) {
		const uint64_t low = mask & (0 - mask);
		if (x & 1) r |= low;
		x >>= 1;
		mask ^= low;
	}
	return r;
}
MSC_HD uint64_t msc_bits_extract(uint64_t x, uint64_t mask) {
	uint64_t r = 0, bit = 1;
	while (mask) {
		const uint64_t low = mask & (0 - mask);
		if (x & low) r |= bit;
		bit <<= 1;
		mask ^= low;
	}
	return r;
}

// where element c of a tile (its destination index gathered under fd) lies in LDS: rows of 2^w elements, the 16-byte chunks of a row
// exchanged by row bits, so that the lanes of a wave, which scatter one source run over 16 rows, do not all meet one bank
MSC_HD uint32_t msc_rc_swizzle(uint32_t c, const MscRcPlan& p, uint32_t lgE) { return c ^ ((((c >> p.w) >> p.swz_shift) & p.swz_mask) << lgE); }

inline uint32_t msc_log2u(uint64_t x) { uint32_t l = 0; while ((1ull << l) < x) l++; return l; }

// for a layout of whole tiles (L.nbins == L.padded_bins) of at least 2^(2w) elements
inline MscRcPlan msc_rc_plan(const MscLayout& L, int k) {
	MscRcPlan p{};
	p.k = k; p.E = L.E; p.R = L.R;
	p.n_bits = 2 * (uint32_t)k;
	p.w = msc_log2u(256 / L.esz);
	const uint64_t z = msc_rc_phys(0, k, L.E, L.R);
	p.fd = (1ull << p.w) - 1;
	for (uint32_t i = 0; i < p.w; i++) p.fd |= msc_rc_phys(1ull << i, k, L.E, L.R) ^ z;
	for (uint32_t i = 0; i < p.n_bits; i++) if (p.fd >> i & 1) p.fs |= msc_rc_phys(1ull << i, k, L.E, L.R) ^ z;
	for (uint64_t m = p.fd; m; m &= m - 1) p.f_bits++;
	const uint32_t lgE = msc_log2u(L.E), chunk_bits = p.w - lgE, row_bits = p.f_bits - p.w;
	// the rows a wave's 16 lanes of one source run scatter to differ in the row bits just under the top lgE ones (the images of the run's chunk bits)
	p.swz_shift = row_bits > lgE + chunk_bits ? row_bits - lgE - chunk_bits : 0;
	p.swz_mask = (1u << (chunk_bits < row_bits ? chunk_bits : row_bits)) - 1;
	return p;
}

// 16-byte chunks of the largest tile of bin type T: 2^(2w) elements
#define MSC_RC_MAX_CHUNKS(T) ((256u / (uint32_t)sizeof(T)) * (256u / (uint32_t)sizeof(T)) / (16u / (uint32_t)sizeof(T)))

// what k_hist_revcomp asks of a plan: a tile inside the slot and within 64 KiB of LDS, at least a wave of 16-byte chunks, 32-bit offsets
inline bool msc_rc_plan_fits(const MscRcPlan& p, const MscLayout& L) {
	if (p.f_bits > p.n_bits || p.n_bits > 32 || p.f_bits > 2 * p.w) return false;
	return (1u << p.f_bits) / L.E >= 64 && ((uint64_t)L.esz << p.f_bits) <= 64 * 1024;
}
