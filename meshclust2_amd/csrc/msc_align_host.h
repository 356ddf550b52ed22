// msc_align_host.h -- what the alignment entry points (msc_align.hip: msc_align_pairs; msc_align_band.hip: msc_align_pairs_banded,
// msc_align_pairs_auto; msc_align_long.hip: their _long namesakes; msc_align_trace.hip: msc_align_pairs_trace) share on the host: the pair
// record, the checks of a call, the plan of the full-grid launches and the queueing of the full-grid and of the banded kernel.
#pragma once
#include <vector>

#include "msc_objects.h"
#include "msc_align.h"

struct AlignPair {
	uint64_t off1, off2;          // byte offsets of the two sequences in the uploaded text
	uint32_t la, lb;
	uint32_t out;                 // the pair's index in the caller's list
	uint32_t band;                // its half-width (k_align_band; k_align_pairs does not read it)
	uint64_t carry;               // offset of its carry range in the scratch buffer, in rows (global-carry launches; k_align_tiles: of its borders)
};

constexpr uint32_t kAlignLdsMax = 160 * 1024;                                       // of a workgroup
constexpr uint32_t kAlignClassTop[] = {8 * 1024, 32 * 1024, 64 * 1024, kAlignLdsMax};          // LDS-carry classes; what needs more keeps its carry in global memory
constexpr int kAlignClasses = 5;
constexpr uint64_t kAlignScratchRows = (512ull << 20) / sizeof(MscAlignTriple);      // carry rows one global-carry launch may use

int msc_align_list(msc_ctx* ctx, const char* who, const uint64_t* offsets, uint64_t n_seqs, const uint32_t* first, const uint32_t* second, uint64_t n_pairs, int match, int mismatch,
                   int gap_open, int gap_continue, std::vector<AlignPair>& pairs, uint64_t& text_bytes, uint32_t max_len = kAlignMaxLen);
// One launch of the full-grid kernel: pairs [at, at + n) of the sorted list, the dynamic LDS it asks for, where its carry lives and (global
// carry) the rows of the scratch buffer it uses
struct AlignLaunch { uint64_t at, n; uint32_t lds; bool lds_carry; uint64_t rows; };
// Sorts `pairs` into the classes of LDS need, longest first inside each, sets their carry offsets and lists the launches (msc_align_queue_full
// and msc_align_pairs_trace queue the same plan)
void msc_align_plan_full(std::vector<AlignPair>& pairs, std::vector<AlignLaunch>& launches, uint64_t& scratch_rows);
int msc_align_queue_full(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out);
int msc_align_queue_banded(msc_ctx* ctx, std::vector<AlignPair>& pairs, const uint8_t* d_text, const MscAlignParams& P, int32_t* d_out, uint64_t n_out);
