// msc_multi_plan.h -- the host arithmetic of the Q x M calls (msc_api_multi.hip, msc_api_pairs.hip): how msc_score_multi cuts its queries
// into blocks, and how a block's candidates are cut into chunks. Free of HIP, so that tests/multi_plan_check.cpp builds it with g++ alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct MscMultiBlock {
	uint64_t q0, nq;          // queries [q0, q0 + nq) of the call
	bool matrix;              // the block runs on the matrix cores
};

// The blocks of one msc_score_multi call. With kb_fit (the matrix cores can take the call) blocks are of 128 consecutive queries, the last
// one short; otherwise of 64. A block of two queries or more is offered to the matrix cores: declines(q0, nq) says whether it stays off them
// (its hot list is too long, or no ranks mirror stands while the earth mover's distance is wanted). A declined block of more than 64 becomes
// consecutive sub-blocks of 64 for the older routes. A trailing block of one query is kept (it takes the per-query route).
template <class Declines>
inline void msc_multi_plan(uint64_t n_q, bool kb_fit, Declines declines, std::vector<MscMultiBlock>& out) {
	out.clear();
	const uint64_t blk = kb_fit ? 128 : 64;
	for (uint64_t q0 = 0; q0 < n_q; q0 += blk) {
		const uint64_t nq = std::min(blk, n_q - q0);
		const bool matrix = kb_fit && nq >= 2 && !declines(q0, nq);
		for (uint64_t s = 0; s < nq; s += matrix ? nq : 64) out.push_back(MscMultiBlock{q0 + s, matrix ? nq : std::min<uint64_t>(64, nq - s), matrix});
	}
}

// The candidate chunks of a block: m candidates, of which `cap` fit one launch's scratch (never taken below 256), in n equal chunks.
struct MscCandChunks { uint64_t chunk, n; };
inline MscCandChunks msc_cand_chunks(uint64_t m, uint64_t cap) {
	const uint64_t c0 = std::min(std::max<uint64_t>(cap, 256), m);
	const uint64_t n = (m + c0 - 1) / c0;
	return MscCandChunks{(m + n - 1) / n, n};
}
