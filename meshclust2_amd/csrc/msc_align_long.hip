// msc_align_long.hip -- msc_align_pairs_long, msc_align_pairs_long_banded and msc_align_pairs_long_auto on the device: the alignments of
// msc_align.hip and msc_align_band.hip for sequences of up to kAlignLongMaxLen bytes (the tiles, the borders and a lane's start
// are msc_align_long.h's, the band, the per-lane step and the certificate msc_align_band.h's, the cell update msc_align.h's).
//
//   k_align_tiles : one TILE per wave (a workgroup is one wave): 256 columns of a stripe by at most H rows of its row window. The wave is the
//       systolic array of k_align_band<4 columns a lane> over WIDE states (a score word, a length word and a count word: nine DPP wave shifts
//       hand a column on). A lane reads its four bytes of the first sequence from global memory; the tile's rows of the second are staged in
//       LDS, H + 128 bytes. The row above the tile comes from the stripe's row border, the column to its left from the pair's column border,
//       both in the pair's range of a scratch buffer the context owns; the tile overwrites both in place with its bottom row and its last
//       column. Launch d of a round runs the tiles with stripe + row block = d of all the round's pairs: the tiles of one launch touch
//       disjoint entries, every entry a tile reads was written by an earlier launch (or is decided by band arithmetic to be a boundary or out
//       of band), and the order of the launches in the stream is the only synchronisation. No atomics, no wave waits for another.
//   The host lists the tiles of a round sorted by launch and uploads the table once; a round takes as many pairs as kAlignScratchRows' bytes
//   of borders (and kAlignRoundTiles table entries) hold: msc_align_plan_tiles (msc_align_plan.h).
//   This file holds the kernel and msc_align_queue_tiles. The entry points are msc_align_api.hip's, and so is the routing: pairs with both
//   lengths within kAlignMaxLen go through msc_align_queue_full / msc_align_queue_banded, so through the kernels of the short entries,
//   unless MSC_ALIGN_LONG_ALL=1 sends every pair here.
#include <cstdio>
#include <vector>

#include "msc_objects.h"
#include "msc_align_long.h"
#include "msc_align_host.h"
#include "msc_align_wave.h"

namespace {

// certified: nullptr for the full grid
__global__ void __launch_bounds__(kAlignLanes) k_align_tiles(const uint8_t* __restrict__ text, const AlignPair* __restrict__ pairs, const AlignTileItem* __restrict__ tiles, uint32_t H,
                                                             MscAlignParams P, MscAlignWideTriple* borders, int32_t* __restrict__ score, int32_t* __restrict__ length,
                                                             int32_t* __restrict__ matches, int32_t* __restrict__ certified) {
	extern __shared__ __attribute__((aligned(16))) unsigned char at_smem[];          // the tile's rows of the second sequence between two pads of kAlignSeqPad zeros
	const AlignTileItem it = tiles[blockIdx.x];
	const AlignPair pr = pairs[it.pair];
	const uint32_t lane = threadIdx.x, la = pr.la, lb = pr.lb, stripes = msc_align_stripes(la);
	const MscAlignBand band = msc_align_long_band(la, lb, pr.band);
	const MscAlignTile tile = msc_align_tile(band, la, lb, it.stripe, it.block, H);
	const uint32_t rows = tile.bot - tile.top + 1;
	for (uint32_t i = lane; i < rows + 2 * kAlignSeqPad; i += kAlignLanes) at_smem[i] = i >= kAlignSeqPad && i < kAlignSeqPad + rows ? text[pr.off2 + (tile.top - 1) + (i - kAlignSeqPad)] : (uint8_t)0;
	__syncthreads();
	MscAlignWideTriple* col_border = borders + pr.carry;
	MscAlignWideTriple* row_border = col_border + msc_align_long_row_at(lb) + (uint64_t)it.stripe * kAlignRowBorder;
	const uint32_t first = tile.c0 + lane * kAlignCols;          // 1-based: the lane's first column
	uint32_t bytes = 0;
#pragma unroll
	for (int c = 0; c < kAlignCols; c++) if (first - 1 + c < la) bytes |= (uint32_t)text[pr.off1 + first - 1 + c] << (8 * c);          // (columns past the end: zeros, computed and never read)
	const int32_t neg_inf = msc_align_neg_inf(la, lb, P);
	const MscAlignWideTriple deep = msc_align_wide_deep();
	MscAlignWideLane L;
	msc_align_tile_start(L, band, tile, lane, bytes, col_border, row_border, neg_inf, P);
	const bool writes = lane == kAlignLanes - 1 && it.stripe + 1 < stripes;
	const uint32_t steps = rows + kAlignLanes - 1;
	MscAlignWideTriple out = L.col[kAlignCols - 1];
	MscAlignWideTriple next = msc_align_tile_left(tile, tile.top, col_border, neg_inf, P);          // what lane 0 receives at the coming step
	for (uint32_t t = 0; t < steps; t++) {
		MscAlignWideTriple recv = shift_triple(out);
		if (lane == 0) recv = next;
		const uint32_t ahead = tile.top + t + 1;                              // (one step ahead: the load is under way while this row is filled)
		next = ahead <= tile.bot ? msc_align_tile_left(tile, ahead, col_border, neg_inf, P) : deep;          // (never a row of another tile: its owner may be writing it)
		const int32_t row = (int32_t)(tile.top + t) - (int32_t)lane;          // 1-based
		const uint32_t b = at_smem[(int32_t)(kAlignSeqPad + t) - (int32_t)lane];
		if (row >= (int32_t)tile.top && row <= (int32_t)tile.bot) {
			msc_align_band_lane_step(L, band, first, (uint32_t)row, recv, b, P);
			if (writes) col_border[row] = L.col[kAlignCols - 1];
		}
		out = L.col[kAlignCols - 1];
	}
	// every lane has ended on row tile.bot
	if (tile.bot < tile.win.r1) {          // a tile follows below: its row above, and its corner (this lane 0's left neighbour at the last row)
#pragma unroll
		for (int c = 0; c < kAlignCols; c++) row_border[1 + lane * kAlignCols + c] = L.col[c];
		if (lane == 0) row_border[0] = L.prev;
	}
	const uint32_t at = (la - 1) % kAlignStripe;
	if (it.stripe + 1 == stripes && tile.bot == lb && lane == at / kAlignCols) {          // the lane that owns column la reports
		MscAlignWideTriple t = L.col[0];
#pragma unroll
		for (int c = 1; c < kAlignCols; c++) if ((uint32_t)c == at % kAlignCols) t = L.col[c];
		const MscAlignStateT<MscAlignWide> r = msc_align_final(t);
		score[pr.out] = r.s;
		length[pr.out] = (int32_t)MscAlignCount<MscAlignWide>::length(r.w);
		matches[pr.out] = (int32_t)MscAlignCount<MscAlignWide>::matches(r.w);
		if (certified) certified[pr.out] = msc_align_band_certified(la, lb, pr.band, P, r.s) ? 1 : 0;
	}
}

}  // namespace

// Queues k_align_tiles for `pairs`, each at its own half-width (kAlignBandNone: the full grid), in rounds: pair p's integers go to d_out[p.out],
// d_out[n_out + p.out], d_out[2 * n_out + p.out] and, where `flags`, its certificate to d_out[3 * n_out + p.out]
int msc_align_queue_tiles(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out, bool flags, uint32_t H) {
	static bool raised = false;
	if (!raised) {
		HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_align_tiles, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kAlignTileRowsMax + 2 * kAlignSeqPad)));
		raised = true;
	}
	AlignTileRound R;
	for (size_t at = 0; at < pairs.size(); at += R.n) {
		msc_align_plan_tiles(pairs, at, H, R);
		if (int r = ensure(ctx, ctx->align_long_pairs, R.n * sizeof(AlignPair))) return r;
		if (int r = ensure(ctx, ctx->align_long_tiles, R.table.size() * sizeof(AlignTileItem))) return r;
		if (int r = ensure(ctx, ctx->align_long_borders, R.triples * sizeof(MscAlignWideTriple))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->align_long_pairs.p, pairs.data() + at, R.n * sizeof(AlignPair), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->align_long_tiles.p, R.table.data(), R.table.size() * sizeof(AlignTileItem), hipMemcpyHostToDevice, ctx->stream));
		const AlignTileItem* d_tiles = (const AlignTileItem*)ctx->align_long_tiles.p;
		for (uint32_t d = 0; d < R.launches; d++) {
			const uint64_t count = R.start[d + 1] - R.start[d];
			if (!count) continue;
			k_align_tiles<<<dim3((unsigned)count), dim3(kAlignLanes), H + 2 * kAlignSeqPad, ctx->stream>>>(d_text, (const AlignPair*)ctx->align_long_pairs.p, d_tiles + R.start[d], H, P,
			                                                                                                (MscAlignWideTriple*)ctx->align_long_borders.p, d_out, d_out + n_out, d_out + 2 * n_out,
			                                                                                                flags ? d_out + 3 * n_out : nullptr);
			HIP_TRY(ctx, hipGetLastError());
		}
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the next round reuses the tables and the borders
	}
	snprintf(ctx->last_kernel_buf, sizeof(ctx->last_kernel_buf), "k_align_tiles<wide states, %u rows a tile>", H);
	ctx->last_kernel = ctx->last_kernel_buf;
	ctx->last_query_tile = 0;
	return MSC_OK;
}
