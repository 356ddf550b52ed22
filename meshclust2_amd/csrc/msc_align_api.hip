// msc_align_api.hip -- the six alignment entry points that return integers: msc_align_pairs, msc_align_pairs_banded,
// msc_align_pairs_auto and their _long namesakes, a few lines each over ONE driver, align_call. What tells them apart is an AlignCall: the
// length limit, whether pairs past kAlignMaxLen (or all, MSC_ALIGN_LONG_ALL=1) may take the tile route, and the mode -- the full grid, one
// half-width for every pair, or msc_align_pairs_auto's loop. A short entry is its _long namesake with the lower limit and the tile route shut.
// The kernels and their queueing are msc_align.hip's, msc_align_band.hip's and msc_align_long.hip's, the plans msc_align_plan.h's.
// msc_align_list and msc_align_download serve msc_align_pairs_trace (msc_align_trace.hip) as well.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msc_objects.h"
#include "msc_align_host.h"

// The checks every alignment call makes on the host before anything is queued, and the pair records in the caller's order
int msc_align_list(msc_ctx* ctx, const char* who, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs, int match, int mismatch,
                   int gap_open, int gap_continue, std::vector<AlignPair>& pairs, uint64_t& text_bytes, uint32_t max_len) {
	if (n_pairs > 0xfffffff0ull) return fail(ctx, MSC_ERR_INVALID_ARG, "%s: too many pairs in one call", who);
	for (int v : {match, mismatch, gap_open, gap_continue})
		if (v > kAlignMaxParam || v < -kAlignMaxParam) return fail(ctx, MSC_ERR_INVALID_ARG, "%s: a scoring parameter of %d (at most %d in absolute value)", who, v, kAlignMaxParam);
	pairs.resize(n_pairs);
	for (uint64_t p = 0; p < n_pairs; p++) {
		AlignPair& a = pairs[p];
		for (uint32_t s : {first[p], second[p]}) {
			if (s >= n_seqs) return fail(ctx, MSC_ERR_INVALID_ARG, "%s: pair %llu names sequence %u of %llu", who, (unsigned long long)p, s, (unsigned long long)n_seqs);
			if (offsets[s + 1] <= offsets[s] || offsets[s + 1] - offsets[s] > max_len)
				return fail(ctx, MSC_ERR_INVALID_ARG, "%s: sequence %u has %lld bytes (1 .. %u)", who, s, (long long)(offsets[s + 1] - offsets[s]), max_len);
		}
		a.off1 = offsets[first[p]]; a.la = (uint32_t)(offsets[first[p] + 1] - a.off1);
		a.off2 = offsets[second[p]]; a.lb = (uint32_t)(offsets[second[p] + 1] - a.off2);
		a.out = (uint32_t)p; a.band = 0; a.carry = 0;
	}
	text_bytes = 0;          // the text up to the end of the last listed sequence
	for (const AlignPair& a : pairs) text_bytes = std::max({text_bytes, a.off1 + a.la, a.off2 + a.lb});
	return MSC_OK;
}

int msc_align_download(msc_ctx* ctx, const int32_t* d_out, uint64_t n_pairs, int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified) {
	std::vector<int32_t> out((certified ? 4 : 3) * n_pairs);          // (the caller's arrays stay untouched unless every launch went through)
	HIP_TRY(ctx, hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	std::copy(out.begin(), out.begin() + n_pairs, score);
	std::copy(out.begin() + n_pairs, out.begin() + 2 * n_pairs, length);
	std::copy(out.begin() + 2 * n_pairs, out.begin() + 3 * n_pairs, matches);
	if (certified) for (uint64_t p = 0; p < n_pairs; p++) certified[p] = out[3 * n_pairs + p] ? 1 : 0;
	return MSC_OK;
}

namespace {

enum class AlignMode { kFull, kBanded, kAuto };
struct AlignCall {
	const char* who;          // the entry's name, for messages
	uint32_t max_len;         // bytes of a listed sequence
	bool tiles;               // the _long entries: pairs past kAlignMaxLen go to k_align_tiles, and the two switches are read
	AlignMode mode;
	uint32_t band;            // kBanded: every pair's half-width. kAuto: first_band
};

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

// One group of launches: the short pairs of `pairs` through the kernels of the short entries, the long ones through k_align_tiles. banded: each
// pair at its own half-width, with its certificate; otherwise the full grid. *tiled: a launch of k_align_tiles ran. A list without a long pair
// (every list of a short entry) is queued as it stands and reordered in place, as the short entries always did: no copy of 20 000 records
int queue_mixed(msc_ctx* ctx, std::vector<AlignPair>& pairs, const LongSwitches& sw, bool banded, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out, bool* tiled) {
	if (!banded) for (AlignPair& a : pairs) a.band = kAlignBandNone;
	std::vector<AlignPair> shorter, large;
	const bool split = std::any_of(pairs.begin(), pairs.end(), [&](const AlignPair& a) { return is_long(a, sw); });
	if (split) for (const AlignPair& a : pairs) (is_long(a, sw) ? large : shorter).push_back(a);
	std::vector<AlignPair>& small = split ? shorter : pairs;
	if (!small.empty()) if (int r = banded ? msc_align_queue_banded(ctx, small, d_text, P, d_out, n_out) : msc_align_queue_full(ctx, small, d_text, P, d_out, n_out)) return r;
	if (!large.empty()) {
		if (int r = msc_align_queue_tiles(ctx, large, d_text, P, d_out, n_out, banded, sw.H)) return r;
		*tiled = true;
	}
	return MSC_OK;
}

void name_tiles(msc_ctx* ctx, const LongSwitches& sw) {          // the call's kernel is the tiled one wherever one of its launches ran
	snprintf(ctx->last_kernel_buf, sizeof(ctx->last_kernel_buf), "k_align_tiles<wide states, %u rows a tile>", sw.H);
	ctx->last_kernel = ctx->last_kernel_buf;
}

// certified: kBanded only. band_used: kAuto only, and may be NULL there
int align_call(msc_ctx* ctx, const AlignCall& call, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs, int match,
               int mismatch, int gap_open, int gap_continue, int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified, uint32_t* band_used) {
	if (!ctx) return MSC_ERR_INVALID_ARG;
	if (n_pairs == 0) return MSC_OK;
	if (!seqs || !offsets || !first || !second || !score || !length || !matches || (call.mode == AlignMode::kBanded && !certified))
		return fail(ctx, MSC_ERR_INVALID_ARG, "%s: a NULL argument", call.who);
	std::vector<AlignPair> all;
	uint64_t text_bytes = 0;
	if (int r = msc_align_list(ctx, call.who, offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open, gap_continue, all, text_bytes, call.max_len)) return r;
	const MscAlignParams P = msc_align_params(match, mismatch, gap_open, gap_continue);
	// (a short entry reads no switch; within its limit no pair is long, so every group of launches below is one queue call)
	const LongSwitches sw = call.tiles ? read_switches() : LongSwitches{false, kAlignTileRows};
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (int r = ensure(ctx, ctx->align_text, text_bytes + 4)) return r;
	if (int r = ensure(ctx, ctx->align_out, (call.mode == AlignMode::kFull ? 3 : 4) * n_pairs * sizeof(int32_t))) return r;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->align_text.p, seqs, text_bytes, hipMemcpyHostToDevice, ctx->stream));
	const uint8_t* d_text = (const uint8_t*)ctx->align_text.p;
	int32_t* d_out = (int32_t*)ctx->align_out.p;
	bool banded = false, tiled = false;          // kAuto: a banded round ran | any mode: a launch of k_align_tiles ran
	char name[sizeof(ctx->last_kernel_buf)] = "";
	std::vector<uint32_t> used;
	if (call.mode != AlignMode::kAuto) {
		for (AlignPair& a : all) a.band = call.band;
		if (int r = queue_mixed(ctx, all, sw, call.mode == AlignMode::kBanded, d_text, P, d_out, n_pairs, &tiled)) return r;
	} else {
		const uint32_t w0 = call.band ? call.band : kAlignBandDefault;
		// a band is worth a run by the rule of the kernel the pair goes to (a long pair's half-width has no cap below its shorter length)
		auto worth = [&](const AlignPair& a) { return is_long(a, sw) ? msc_align_long_worth(a.la, a.lb, a.band) : msc_align_band_worth(a.la, a.lb, a.band); };
		used.assign(n_pairs, kAlignBandNone);
		std::vector<AlignPair> open, full;          // the pairs of the coming banded round, each at its own band | those a band does not help
		const bool offered = msc_align_band_offered(P);
		for (AlignPair a : all) {
			a.band = w0;
			(offered && worth(a) ? open : full).push_back(a);
		}
		std::vector<int32_t> flags(n_pairs);
		while (!open.empty()) {
			if (int r = queue_mixed(ctx, open, sw, true, d_text, P, d_out, n_pairs, &tiled)) return r;
			HIP_TRY(ctx, hipMemcpyAsync(flags.data(), d_out + 3 * n_pairs, n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
			HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			banded = true;
			snprintf(name, sizeof(name), "%s", ctx->last_kernel_buf);
			std::vector<AlignPair> again;
			for (AlignPair a : open) {
				if (flags[a.out]) { used[a.out] = a.band; continue; }
				// (a first_band near 2^32 must not wrap; past the lengths it is worth nothing. A short pair is worth a run only at a band below its
				// shorter length, at most 32 766, so it never meets the clamp)
				a.band = a.band > kAlignLongMaxLen ? 2 * kAlignLongMaxLen : a.band * 2;
				(worth(a) ? again : full).push_back(a);
			}
			open.swap(again);
		}
		if (!full.empty()) if (int r = queue_mixed(ctx, full, sw, false, d_text, P, d_out, n_pairs, &tiled)) return r;
	}
	if (int r = msc_align_download(ctx, d_out, n_pairs, score, length, matches, call.mode == AlignMode::kBanded ? certified : nullptr)) return r;
	if (band_used) std::copy(used.begin(), used.end(), band_used);
	if (tiled) name_tiles(ctx, sw);
	else if (banded) {          // the call's kernel is the banded one wherever a round ran
		snprintf(ctx->last_kernel_buf, sizeof(ctx->last_kernel_buf), "%s", name);
		ctx->last_kernel = ctx->last_kernel_buf;
	}
	return MSC_OK;
}

}  // namespace

extern "C" int msc_align_pairs(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                               int match, int mismatch, int gap_open, int gap_continue, int32_t* score, int32_t* length, int32_t* matches) {
	return align_call(ctx, {"msc_align_pairs", kAlignMaxLen, false, AlignMode::kFull, kAlignBandNone}, seqs, offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open, gap_continue,
	                  score, length, matches, nullptr, nullptr);
}
extern "C" int msc_align_pairs_banded(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                      int match, int mismatch, int gap_open, int gap_continue, uint32_t band, int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified) {
	return align_call(ctx, {"msc_align_pairs_banded", kAlignMaxLen, false, AlignMode::kBanded, band}, seqs, offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open, gap_continue,
	                  score, length, matches, certified, nullptr);
}
extern "C" int msc_align_pairs_auto(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                    int match, int mismatch, int gap_open, int gap_continue, uint32_t first_band, int32_t* score, int32_t* length, int32_t* matches, uint32_t* band_used) {
	return align_call(ctx, {"msc_align_pairs_auto", kAlignMaxLen, false, AlignMode::kAuto, first_band}, seqs, offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open, gap_continue,
	                  score, length, matches, nullptr, band_used);
}
extern "C" int msc_align_pairs_long(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                    int match, int mismatch, int gap_open, int gap_continue, int32_t* score, int32_t* length, int32_t* matches) {
	return align_call(ctx, {"msc_align_pairs_long", kAlignLongMaxLen, true, AlignMode::kFull, kAlignBandNone}, seqs, offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open,
	                  gap_continue, score, length, matches, nullptr, nullptr);
}
extern "C" int msc_align_pairs_long_banded(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                           int match, int mismatch, int gap_open, int gap_continue, uint32_t band, int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified) {
	return align_call(ctx, {"msc_align_pairs_long_banded", kAlignLongMaxLen, true, AlignMode::kBanded, band}, seqs, offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open,
	                  gap_continue, score, length, matches, certified, nullptr);
}
extern "C" int msc_align_pairs_long_auto(msc_ctx* ctx, const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                                         int match, int mismatch, int gap_open, int gap_continue, uint32_t first_band, int32_t* score, int32_t* length, int32_t* matches, uint32_t* band_used) {
	return align_call(ctx, {"msc_align_pairs_long_auto", kAlignLongMaxLen, true, AlignMode::kAuto, first_band}, seqs, offsets, n_seqs, first, second, n_pairs, match, mismatch, gap_open,
	                  gap_continue, score, length, matches, nullptr, band_used);
}
