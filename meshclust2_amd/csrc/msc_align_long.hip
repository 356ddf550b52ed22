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
//   of borders (and kAlignRoundTiles table entries) hold. Pairs with both lengths within kAlignMaxLen go through msc_align_queue_full /
//   msc_align_queue_banded, so through the kernels of the short entries, unless MSC_ALIGN_LONG_ALL=1 sends every pair here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msc_objects.h"
#include "msc_align_long.h"
#include "msc_align_host.h"

namespace {

constexpr uint64_t kAlignRoundTiles = 16ull << 20;          // table entries of one round (a single pair may need more: it gets a round of its own)

struct AlignTileItem {
	uint32_t pair, stripe, block;
};

__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }          // wave_shr:1

__device__ __forceinline__ MscAlignStateT<MscAlignWide> shift_state(const MscAlignStateT<MscAlignWide>& s) {
	MscAlignStateT<MscAlignWide> r;
	r.s = (int32_t)wave_shr1((uint32_t)s.s); r.w.len = wave_shr1(s.w.len); r.w.cnt = wave_shr1(s.w.cnt);
	return r;
}
__device__ __forceinline__ MscAlignWideTriple shift_triple(const MscAlignWideTriple& t) {
	MscAlignWideTriple r;
	r.m = shift_state(t.m); r.l = shift_state(t.l); r.u = shift_state(t.u);
	return r;
}

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

struct LongSwitches {
	bool all;          // MSC_ALIGN_LONG_ALL=1: every pair of the call goes to k_align_tiles
	uint32_t H;        // MSC_ALIGN_TILE_ROWS
};
LongSwitches read_switches() {          // on every call: tests flip them inside one process
	LongSwitches s{false, kAlignTileRows};
	if (const char* v = getenv("MSC_ALIGN_LONG_ALL")) s.all = v[0] == '1';
	if (const char* v = getenv("MSC_ALIGN_TILE_ROWS")) {
		const long n = atol(v);
		if (n > 0) s.H = (uint32_t)std::min<long>(std::max<long>(n, kAlignTileRowsMin), kAlignTileRowsMax);
	}
	return s;
}
bool is_long(const AlignPair& a, const LongSwitches& sw) { return sw.all || a.la > kAlignMaxLen || a.lb > kAlignMaxLen; }

// Queues k_align_tiles for `pairs`, each at its own half-width (kAlignBandNone: the full grid), in rounds: pair p's integers go to d_out[p.out],
// d_out[n_out + p.out], d_out[2 * n_out + p.out] and, where `flags`, its certificate to d_out[3 * n_out + p.out]
int queue_tiles(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out, bool flags, uint32_t H) {
	const uint64_t budget = kAlignScratchRows * sizeof(MscAlignTriple) / sizeof(MscAlignWideTriple);          // triples of borders a round may use
	auto tiles_of = [&](const AlignPair& a) {
		const MscAlignBand band = msc_align_long_band(a.la, a.lb, a.band);
		uint64_t n = 0;
		for (uint32_t s = 0; s < msc_align_stripes(a.la); s++) {
			const MscAlignWindow win = msc_align_band_window(band, a.la, a.lb, s * kAlignStripe + 1, kAlignStripe);
			n += msc_align_last_block(win, H) - msc_align_first_block(win, H) + 1;
		}
		return n;
	};
	static bool raised = false;
	if (!raised) {
		HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_align_tiles, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kAlignTileRowsMax + 2 * kAlignSeqPad)));
		raised = true;
	}
	std::vector<AlignTileItem> table;
	std::vector<uint64_t> start;          // where launch d's tiles begin in the table
	for (size_t at = 0; at < pairs.size();) {
		size_t n = 0;
		uint64_t triples = 0, n_tiles = 0;
		for (; at + n < pairs.size(); n++) {
			AlignPair& a = pairs[at + n];
			const uint64_t need = msc_align_long_borders(a.la, a.lb), t = tiles_of(a);
			if (n && (triples + need > budget || n_tiles + t > kAlignRoundTiles)) break;
			a.carry = triples;
			triples += need;
			n_tiles += t;
		}
		// the round's tiles, sorted by launch: count, then place
		uint32_t launches = 0;
		for (size_t k = 0; k < n; k++) {
			const AlignPair& a = pairs[at + k];
			launches = std::max(launches, msc_align_stripes(a.la) + (a.lb - 1) / H);
		}
		start.assign((size_t)launches + 1, 0);
		table.resize(n_tiles);
		for (int pass = 0; pass < 2; pass++) {
			for (size_t k = 0; k < n; k++) {
				const AlignPair& a = pairs[at + k];
				const MscAlignBand band = msc_align_long_band(a.la, a.lb, a.band);
				for (uint32_t s = 0; s < msc_align_stripes(a.la); s++) {
					const MscAlignWindow win = msc_align_band_window(band, a.la, a.lb, s * kAlignStripe + 1, kAlignStripe);
					for (uint32_t b = msc_align_first_block(win, H); b <= msc_align_last_block(win, H); b++) {
						if (pass == 0) start[s + b + 1]++;
						else table[start[s + b]++] = AlignTileItem{(uint32_t)k, s, b};
					}
				}
			}
			if (pass == 0) for (uint32_t d = 0; d < launches; d++) start[d + 1] += start[d];
			else { for (uint32_t d = launches; d > 0; d--) start[d] = start[d - 1]; start[0] = 0; }          // (placing moved every start to its launch's end)
		}
		if (int r = ensure(ctx, ctx->align_long_pairs, n * sizeof(AlignPair))) return r;
		if (int r = ensure(ctx, ctx->align_long_tiles, n_tiles * sizeof(AlignTileItem))) return r;
		if (int r = ensure(ctx, ctx->align_long_borders, triples * sizeof(MscAlignWideTriple))) return r;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->align_long_pairs.p, pairs.data() + at, n * sizeof(AlignPair), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->align_long_tiles.p, table.data(), n_tiles * sizeof(AlignTileItem), hipMemcpyHostToDevice, ctx->stream));
		const AlignTileItem* d_tiles = (const AlignTileItem*)ctx->align_long_tiles.p;
		for (uint32_t d = 0; d < launches; d++) {
			const uint64_t count = start[d + 1] - start[d];
			if (!count) continue;
			k_align_tiles<<<dim3((unsigned)count), dim3(kAlignLanes), H + 2 * kAlignSeqPad, ctx->stream>>>(d_text, (const AlignPair*)ctx->align_long_pairs.p, d_tiles + start[d], H, P,
			                                                                                                (MscAlignWideTriple*)ctx->align_long_borders.p, d_out, d_out + n_out, d_out + 2 * n_out,
			                                                                                                flags ? d_out + 3 * n_out : nullptr);
			HIP_TRY(ctx, hipGetLastError());
		}
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the next round reuses the tables and the borders
		at += n;
	}
	snprintf(ctx->last_kernel_buf, sizeof(ctx->last_kernel_buf), "k_align_tiles<wide states, %u rows a tile>", H);
	ctx->last_kernel = ctx->last_kernel_buf;
	ctx->last_query_tile = 0;
	return MSC_OK;
}

// One group of launches: the short pairs of `pairs` through the kernels of the short entries, the long ones through k_align_tiles. banded: each
// pair at its own half-width, with its certificate; otherwise the full grid. *tiled: a launch of k_align_tiles ran
int queue_mixed(msc_ctx* ctx, const std::vector<AlignPair>& pairs, const LongSwitches& sw, bool banded, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out,
                bool* tiled) {
	std::vector<AlignPair> small, large;
	for (AlignPair a : pairs) {
		if (!banded) a.band = kAlignBandNone;
		(is_long(a, sw) ? large : small).push_back(a);
	}
	if (!small.empty()) if (int r = banded ? msc_align_queue_banded(ctx, small, d_text, P, d_out, n_out) : msc_align_queue_full(ctx, small, d_text, P, d_out, n_out)) return r;
	if (!large.empty()) {
		if (int r = queue_tiles(ctx, large, d_text, P, d_out, n_out, banded, sw.H)) return r;
		*tiled = true;
	}
	return MSC_OK;
}

void name_tiles(msc_ctx* ctx, const LongSwitches& sw) {          // the call's kernel is the tiled one wherever one of its launches ran
	snprintf(ctx->last_kernel_buf, sizeof(ctx->last_kernel_buf), "k_align_tiles<wide states, %u rows a tile>", sw.H);
	ctx->last_kernel = ctx->last_kernel_buf;
}

}  // namespace

extern "C" int msc_align_pairs_long(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                    int match, int mismatch, int gap_open, int gap_continue, int32_t* score, int32_t* length, int32_t* matches) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (n_pairs == 0) return MSC_OK;
	if (!seqs || !offsets || !first || !second || !score || !length || !matches) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_align_pairs_long: a NULL argument");
	std::vector<AlignPair> pairs;
	uint64_t text_bytes = 0;
	if (int r = msc_align_list(ctx, "msc_align_pairs_long", offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open, gap_continue, pairs, text_bytes, kAlignLongMaxLen)) return r;
	const LongSwitches sw = read_switches();
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (int r = ensure(ctx, ctx->align_text, text_bytes + 4)) return r;
	if (int r = ensure(ctx, ctx->align_out, 3 * n_pairs * sizeof(int32_t))) return r;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->align_text.p, seqs, text_bytes, hipMemcpyHostToDevice, ctx->stream));
	int32_t* d_out = (int32_t*)ctx->align_out.p;
	bool tiled = false;
	if (int r = queue_mixed(ctx, pairs, sw, false, (const uint8_t*)ctx->align_text.p, msc_align_params(match, mismatch, gap_open, gap_continue), d_out, n_pairs, &tiled)) return r;
	std::vector<int32_t> out(3 * n_pairs);          // (the caller's arrays stay untouched unless every launch went through)
	HIP_TRY(ctx, hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	std::copy(out.begin(), out.begin() + n_pairs, score);
	std::copy(out.begin() + n_pairs, out.begin() + 2 * n_pairs, length);
	std::copy(out.begin() + 2 * n_pairs, out.end(), matches);
	if (tiled) name_tiles(ctx, sw);
	return MSC_OK;
}

extern "C" int msc_align_pairs_long_banded(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                           int match, int mismatch, int gap_open, int gap_continue, uint32_t band, int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (n_pairs == 0) return MSC_OK;
	if (!seqs || !offsets || !first || !second || !score || !length || !matches || !certified) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_align_pairs_long_banded: a NULL argument");
	std::vector<AlignPair> pairs;
	uint64_t text_bytes = 0;
	if (int r = msc_align_list(ctx, "msc_align_pairs_long_banded", offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open, gap_continue, pairs, text_bytes, kAlignLongMaxLen))
		return r;
	for (AlignPair& a : pairs) a.band = band;
	const LongSwitches sw = read_switches();
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (int r = ensure(ctx, ctx->align_text, text_bytes + 4)) return r;
	if (int r = ensure(ctx, ctx->align_out, 4 * n_pairs * sizeof(int32_t))) return r;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->align_text.p, seqs, text_bytes, hipMemcpyHostToDevice, ctx->stream));
	int32_t* d_out = (int32_t*)ctx->align_out.p;
	bool tiled = false;
	if (int r = queue_mixed(ctx, pairs, sw, true, (const uint8_t*)ctx->align_text.p, msc_align_params(match, mismatch, gap_open, gap_continue), d_out, n_pairs, &tiled)) return r;
	std::vector<int32_t> out(4 * n_pairs);          // (the caller's arrays stay untouched unless every launch went through)
	HIP_TRY(ctx, hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	std::copy(out.begin(), out.begin() + n_pairs, score);
	std::copy(out.begin() + n_pairs, out.begin() + 2 * n_pairs, length);
	std::copy(out.begin() + 2 * n_pairs, out.begin() + 3 * n_pairs, matches);
	for (uint64_t p = 0; p < n_pairs; p++) certified[p] = out[3 * n_pairs + p] ? 1 : 0;
	if (tiled) name_tiles(ctx, sw);
	return MSC_OK;
}

extern "C" int msc_align_pairs_long_auto(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                         int match, int mismatch, int gap_open, int gap_continue, uint32_t first_band, int32_t* score, int32_t* length, int32_t* matches, uint32_t* band_used) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (n_pairs == 0) return MSC_OK;
	if (!seqs || !offsets || !first || !second || !score || !length || !matches) return fail(ctx, MSC_ERR_INVALID_ARG, "msc_align_pairs_long_auto: a NULL argument");
	std::vector<AlignPair> all;
	uint64_t text_bytes = 0;
	if (int r = msc_align_list(ctx, "msc_align_pairs_long_auto", offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open, gap_continue, all, text_bytes, kAlignLongMaxLen)) return r;
	const MscAlignParams P = msc_align_params(match, mismatch, gap_open, gap_continue);
	const uint32_t w0 = first_band ? first_band : kAlignBandDefault;
	const LongSwitches sw = read_switches();
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (int r = ensure(ctx, ctx->align_text, text_bytes + 4)) return r;
	if (int r = ensure(ctx, ctx->align_out, 4 * n_pairs * sizeof(int32_t))) return r;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->align_text.p, seqs, text_bytes, hipMemcpyHostToDevice, ctx->stream));
	const uint8_t* d_text = (const uint8_t*)ctx->align_text.p;
	int32_t* d_out = (int32_t*)ctx->align_out.p;
	// a band is worth a run by the rule of the kernel the pair goes to (a long pair's half-width has no cap below its shorter length)
	auto worth = [&](const AlignPair& a) { return is_long(a, sw) ? msc_align_long_worth(a.la, a.lb, a.band) : msc_align_band_worth(a.la, a.lb, a.band); };
	std::vector<uint32_t> used(n_pairs, kAlignBandNone);
	std::vector<AlignPair> open, full;          // the pairs of the coming banded round, each at its own band | those a band does not help
	const bool offered = msc_align_band_offered(P);
	for (AlignPair a : all) {
		a.band = w0;
		(offered && worth(a) ? open : full).push_back(a);
	}
	std::vector<int32_t> flags(n_pairs);
	bool banded = false, tiled = false;
	char name[sizeof(ctx->last_kernel_buf)] = "";
	while (!open.empty()) {
		if (int r = queue_mixed(ctx, open, sw, true, d_text, P, d_out, n_pairs, &tiled)) return r;
		HIP_TRY(ctx, hipMemcpyAsync(flags.data(), d_out + 3 * n_pairs, n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		banded = true;
		snprintf(name, sizeof(name), "%s", ctx->last_kernel_buf);
		std::vector<AlignPair> again;
		for (AlignPair a : open) {
			if (flags[a.out]) { used[a.out] = a.band; continue; }
			a.band = a.band > kAlignLongMaxLen ? 2 * kAlignLongMaxLen : a.band * 2;          // (a first_band near 2^32 must not wrap; past the lengths it is worth nothing)
			(worth(a) ? again : full).push_back(a);
		}
		open.swap(again);
	}
	if (!full.empty()) if (int r = queue_mixed(ctx, full, sw, false, d_text, P, d_out, n_pairs, &tiled)) return r;
	std::vector<int32_t> out(3 * n_pairs);          // (the caller's arrays stay untouched unless every launch went through)
	HIP_TRY(ctx, hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	std::copy(out.begin(), out.begin() + n_pairs, score);
	std::copy(out.begin() + n_pairs, out.begin() + 2 * n_pairs, length);
	std::copy(out.begin() + 2 * n_pairs, out.end(), matches);
	if (band_used) std::copy(used.begin(), used.end(), band_used);
	if (tiled) name_tiles(ctx, sw);
	else if (banded) {          // as msc_align_pairs_auto: the banded kernel wherever a round ran
		snprintf(ctx->last_kernel_buf, sizeof(ctx->last_kernel_buf), "%s", name);
		ctx->last_kernel = ctx->last_kernel_buf;
	}
	return MSC_OK;
}
