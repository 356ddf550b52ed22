// align_schedule_check.cpp -- the schedule of k_align_pairs (meshclust2_amd/csrc/msc_align.hip) replayed serially on the host, over the cell
// update, the boundaries and the per-lane step of msc_align.h that the kernel itself compiles: stripes of kAlignStripe columns, 64 lanes
// staggered by one row, the hand-over of a lane's last column to the next lane, the carry column written by the last lane and read back in
// place (one row ahead) by lane 0 of the next stripe, the zero padding of the two sequences, length << 16 | count in one word.
//
//   align_schedule_check pairs.txt        (the dump of tests/align_util.py: write_dump, with results)
//
// Prints the first pair whose (score, length, matches) differ from the dump's and exits 1; exits 0 when every pair agrees. Built by
// tests/test_align_cpu.py with -fsanitize=address,undefined: an index outside the staged sequences or the carry column ends the run.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "msc_align.h"

namespace {

struct Result {
	int32_t score, length, matches;
};

Result run_pair(const std::string& a, const std::string& b, const MscAlignParams& P) {
	const uint32_t la = (uint32_t)a.size(), lb = (uint32_t)b.size(), stripes = msc_align_stripes(la);
	// the workgroup's LDS, byte for byte: exact sizes, so that the sanitizer sees every access past them
	std::vector<uint8_t> lds(msc_align_carry_at(la, lb) + msc_align_carry_bytes(la, lb));
	uint8_t* s1 = lds.data();
	uint8_t* s2 = lds.data() + msc_align_seq2_at(la) + kAlignSeqPad;
	for (uint32_t i = 0; i < stripes * kAlignStripe; i++) s1[i] = i < la ? (uint8_t)a[i] : (uint8_t)0;
	for (uint32_t i = 0; i < lb + 2 * kAlignSeqPad; i++) s2[(int32_t)i - (int32_t)kAlignSeqPad] = i >= kAlignSeqPad && i < kAlignSeqPad + lb ? (uint8_t)b[i - kAlignSeqPad] : (uint8_t)0;
	std::vector<MscAlignTriple> carry(stripes > 1 ? lb + 1 : 0);          // (the kernel keeps it in LDS or in global memory: the same rows either way)
	const int32_t neg_inf = msc_align_neg_inf(la, lb, P);
	const uint32_t steps = lb + kAlignLanes - 1;
	std::vector<MscAlignLane> lanes(kAlignLanes);
	std::vector<MscAlignTriple> out(kAlignLanes), recv(kAlignLanes);
	for (uint32_t s = 0; s < stripes; s++) {
		for (uint32_t lane = 0; lane < (uint32_t)kAlignLanes; lane++) {
			const uint32_t first = s * kAlignStripe + lane * kAlignCols;
			uint32_t bytes;
			memcpy(&bytes, s1 + first, 4);
			msc_align_lane_init(lanes[lane], first + 1, bytes, neg_inf, P);
			out[lane] = lanes[lane].col[kAlignCols - 1];
		}
		MscAlignTriple next = s ? carry.at(1) : msc_align_col0(1, neg_inf, P);
		for (uint32_t t = 0; t < steps; t++) {
			for (uint32_t lane = kAlignLanes - 1; lane >= 1; lane--) recv[lane] = out[lane - 1];          // the wave shift
			recv[0] = next;
			const uint32_t ahead = t + 2 <= lb ? t + 2 : lb;
			next = s ? carry.at(ahead) : msc_align_col0(ahead, neg_inf, P);
			for (uint32_t lane = 0; lane < (uint32_t)kAlignLanes; lane++) {
				const int32_t row = (int32_t)t - (int32_t)lane;
				const uint32_t byte = s2[row];
				if (row >= 0 && row < (int32_t)lb) {
					msc_align_lane_step(lanes[lane], recv[lane], byte, P);
					if (lane == (uint32_t)kAlignLanes - 1 && s + 1 < stripes) carry.at(row + 1) = lanes[lane].col[kAlignCols - 1];
				}
				out[lane] = lanes[lane].col[kAlignCols - 1];
			}
		}
	}
	const uint32_t at = (la - 1) % kAlignStripe;
	const MscAlignState r = msc_align_final(lanes[at / kAlignCols].col[at % kAlignCols]);
	return Result{r.s, (int32_t)(r.w >> 16), (int32_t)(r.w & 0xffffu)};
}

}  // namespace

int main(int argc, char** argv) {
	if (argc != 2) { fprintf(stderr, "usage: align_schedule_check pairs.txt\n"); return 2; }
	std::ifstream in(argv[1]);
	size_t n_seqs = 0, n_sets = 0, n_pairs = 0;
	in >> n_seqs >> n_sets >> n_pairs;
	std::vector<std::string> seqs(n_seqs);
	for (auto& s : seqs) in >> s;
	std::vector<int> par(4 * n_sets);
	for (auto& v : par) in >> v;
	std::vector<uint32_t> pr(2 * n_pairs);
	for (auto& v : pr) in >> v;
	std::vector<Result> want(n_sets * n_pairs);
	for (auto& w : want) in >> w.score >> w.length >> w.matches;
	if (!in || n_pairs == 0) { fprintf(stderr, "align_schedule_check: %s is not a complete dump\n", argv[1]); return 2; }
	for (size_t s = 0; s < n_sets; s++) {
		const MscAlignParams P = msc_align_params(par[4 * s], par[4 * s + 1], par[4 * s + 2], par[4 * s + 3]);
		for (size_t p = 0; p < n_pairs; p++) {
			if (pr[2 * p] >= n_seqs || pr[2 * p + 1] >= n_seqs) { fprintf(stderr, "align_schedule_check: pair %zu names a sequence past the list\n", p); return 2; }
			const Result got = run_pair(seqs[pr[2 * p]], seqs[pr[2 * p + 1]], P), &w = want[s * n_pairs + p];
			if (got.score != w.score || got.length != w.length || got.matches != w.matches) {
				printf("set %zu pair %zu (%zu x %zu): got %d %d %d, the dump holds %d %d %d\n", s, p, seqs[pr[2 * p]].size(), seqs[pr[2 * p + 1]].size(), got.score, got.length,
				       got.matches, w.score, w.length, w.matches);
				return 1;
			}
		}
	}
	printf("%zu pairs under %zu parameter sets agree\n", n_pairs, n_sets);
	return 0;
}
