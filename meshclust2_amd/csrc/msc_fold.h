// msc_fold.h -- the fold map of the folded presence mirror (msc_pair_gemm.hip), shared by the kernels and host code.
//
// A histogram of 4^k bins is folded F-to-1 (F a power of two) by keeping the low digits of the bin: bin -> bin mod (4^k / F). The F bins
// that share a folded bin lie 4^k / F apart, so super-step s of the folded mirror is the OR of super-steps s + j nss / F (j < F) of the
// true one. The map is applied to PHYSICAL positions (msc_layout.h); a set is folded only when 4^k / F is a whole number of tiles, and
// then the tile permutation -- local to a tile -- commutes with the map: fold(phys(b)) = phys(fold(b)), the position inside the tile is
// kept and the tile index is reduced. (The dropped digits are the FIRST bases of the k-mer: two k-mers collide when they agree in their
// last k - log4(F) bases.)
#pragma once
#include <stdint.h>

#include "msc_layout.h"

MSC_HD uint64_t msc_fold_bin_of(uint64_t bin, uint64_t nbins, uint32_t fold) { return fold > 1 ? bin & (nbins / fold - 1) : bin; }

// Whether a set of this layout can be folded by `fold`: 8, 16 or 32; histograms of whole tiles; 4^k / F a whole number of tiles and of
// the 256-bin super-steps the product and k_kb_gather walk (msc_launch_pair_gemm's rule for one slice). k = 5 (1 024 bins) never fits.
MSC_HD bool msc_fold_fits(const MscLayout& L, uint32_t fold) {
	if (fold != 8 && fold != 16 && fold != 32) return false;
	if (L.nbins != L.padded_bins || (L.nbins & (L.nbins - 1))) return false;
	const uint64_t nf = L.nbins / fold;
	return nf >= 256 && nf % 256 == 0 && nf % L.tile_bins == 0;
}
