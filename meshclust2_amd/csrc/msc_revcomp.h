// msc_revcomp.h -- the bin of the reverse complement of a k-mer, shared by the kernels of msc_revcomp.hip and host code.
//
// A = 0, C = 1, G = 2, T = 3; a k-mer x0 .. x(k-1) has bin sum xi * 4^(k-1-i), first base most significant (the order of msc_hist_download).
// The reverse complement reads the complemented bases back to front: its digit of weight 4^j is 3 - (the digit of weight 4^(k-1-j)). As
// bits: reverse all 64, swap the two bits of every pair back (a digit keeps its own bit order), shift the 2k bits down, complement them.
// An involution; a palindromic k-mer (ACGT, AATT) maps to itself, and odd k has none (the middle digit d would have to equal 3 - d).
#pragma once
#include <stdint.h>

#include "msc_layout.h"

MSC_HD uint64_t msc_rc_bin(uint64_t bin, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
	uint64_t x = __brevll(bin);
#else
	uint64_t x = bin;
	x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
	x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
	x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
	x = ((x >> 8) & 0x00ff00ff00ff00ffull) | ((x & 0x00ff00ff00ff00ffull) << 8);
	x = ((x >> 16) & 0x0000ffff0000ffffull) | ((x & 0x0000ffff0000ffffull) << 16);
	x = (x >> 32) | (x << 32);
#endif
	x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
	const int bits = 2 * k;          // 1 <= k <= 32
	x = ~(x >> (64 - bits));
	return bits >= 64 ? x : x & ((1ull << bits) - 1);
}
