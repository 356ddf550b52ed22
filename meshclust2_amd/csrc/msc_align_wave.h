// msc_align_wave.h -- what the alignment kernels share on the device: the hand-over of a lane's last column to the next lane (k_align_pairs,
// k_align_pairs_dirs, k_align_band, k_align_tiles). Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "msc_align.h"

namespace {

__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }          // wave_shr:1
__device__ __forceinline__ MscAlignWide wave_shr1(MscAlignWide w) { return MscAlignWide{wave_shr1(w.len), wave_shr1(w.cnt)}; }

// lane l receives lane l - 1's triple: two DPP wave shifts a state over the packed count word, three over the wide one
template <class W>
__device__ __forceinline__ MscAlignStateT<W> shift_state(const MscAlignStateT<W>& s) {
	MscAlignStateT<W> r;
	r.s = (int32_t)wave_shr1((uint32_t)s.s); r.w = wave_shr1(s.w);
	return r;
}
template <class W>
__device__ __forceinline__ MscAlignTripleT<W> shift_triple(const MscAlignTripleT<W>& t) {
	MscAlignTripleT<W> r;
	r.m = shift_state(t.m); r.l = shift_state(t.l); r.u = shift_state(t.u);
	return r;
}

}  // namespace
