// msc_align_host.h -- what the alignment entry points share on the host. msc_align_api.hip holds the six integer entries (msc_align_pairs,
// _banded, _auto and their _long namesakes) over one driver, msc_align_trace.hip holds msc_align_pairs_trace; both check a call with
// msc_align_list, plan with msc_align_plan.h and fan the integers out with msc_align_download. The queueing of a kernel stays in the file of
// that kernel: msc_align.hip, msc_align_band.hip, msc_align_long.hip.
#pragma once
#include <vector>

#include "msc_objects.h"
#include "msc_align_plan.h"

// The checks every alignment call makes on the host before anything is queued, and the pair records in the caller's order
int msc_align_list(msc_ctx* ctx, const char* who, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs, int match, int mismatch,
                   int gap_open, int gap_continue, std::vector<AlignPair>& pairs, uint64_t& text_bytes, uint32_t max_len = kAlignMaxLen);
// Waits for the stream and hands the caller columns 0 .. 2 of d_out (n_pairs integers each) and, where `certified`, column 3 as flags: the
// caller's arrays stay untouched unless every launch went through
int msc_align_download(msc_ctx* ctx, const int32_t* d_out, uint64_t n_pairs, int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified);
// Each queues one kernel for `pairs` (reordered there) over the uploaded text: pair p's integers go to d_out[p.out], d_out[n_out + p.out] and
// d_out[2 * n_out + p.out], its certificate (the banded kernel; the tiles where `flags`) to d_out[3 * n_out + p.out]
int msc_align_queue_full(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out);
int msc_align_queue_banded(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out);
int msc_align_queue_tiles(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out, bool flags, uint32_t H);
