// align_trace_schedule_check.cpp -- k_align_pairs_dirs, k_align_trace_count and k_align_trace_write (meshclust2_amd/csrc/msc_align_trace.hip)
// replayed serially on the host over the text the kernels compile: the cell update with its decisions and the per-lane step of msc_align.h,
// the layout of the back pointers and the walk of msc_align_trace.h. The forward pass is k_align_pairs's schedule (stripes of kAlignStripe
// columns, 64 lanes staggered by one row, the carry column) with the kernel's one store per lane and step; the two walks run as the kernels
// run them, the first counting the runs, the second writing them back to front into a range of exactly that size.
//
//   align_trace_schedule_check pairs.txt        (the dump of tests/align_trace_util.py: write_dump)
//
// Prints the first pair whose runs differ from the dump's and exits 1; exits 0 when every pair agrees. Built by tests/test_align_trace_cpu.py
// with -fsanitize=address,undefined: the direction buffer and the op range have their exact sizes, so an index outside either ends the run.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "msc_align.h"
#include "msc_align_trace.h"

namespace {

std::vector<uint32_t> run_pair(const std::string& a, const std::string& b, const MscAlignParams& P) {
	const uint32_t la = (uint32_t)a.size(), lb = (uint32_t)b.size(), stripes = msc_align_stripes(la);
	std::vector<uint8_t> lds(msc_align_carry_at(la, lb) + msc_align_carry_bytes(la, lb));
	uint8_t* s1 = lds.data();
	uint8_t* s2 = lds.data() + msc_align_seq2_at(la) + kAlignSeqPad;
	for (uint32_t i = 0; i < stripes * kAlignStripe; i++) s1[i] = i < la ? (uint8_t)a[i] : (uint8_t)0;
	for (uint32_t i = 0; i < lb + 2 * kAlignSeqPad; i++) s2[(int32_t)i - (int32_t)kAlignSeqPad] = i >= kAlignSeqPad && i < kAlignSeqPad + lb ? (uint8_t)b[i - kAlignSeqPad] : (uint8_t)0;
	std::vector<MscAlignTriple> carry(stripes > 1 ? lb + 1 : 0);
	std::vector<uint16_t> dirs(msc_align_trace_words(la, lb), 0xffffu);          // (what no lane stores would send a walk astray)
	const int32_t neg_inf = msc_align_neg_inf(la, lb, P);
	const uint32_t steps = msc_align_trace_steps(lb);
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
					const uint32_t d = msc_align_lane_step_dir(lanes[lane], recv[lane], byte, P);
					dirs.at(msc_align_trace_word_at(lb, s, t, lane)) = (uint16_t)d;
					if (lane == (uint32_t)kAlignLanes - 1 && s + 1 < stripes) carry.at(row + 1) = lanes[lane].col[kAlignCols - 1];
				}
				out[lane] = lanes[lane].col[kAlignCols - 1];
			}
		}
	}
	const uint32_t at = (la - 1) % kAlignStripe;
	uint32_t start = 0;
	msc_align_final_dir(lanes[at / kAlignCols].col[at % kAlignCols], start);
	const uint8_t* t1 = reinterpret_cast<const uint8_t*>(a.data());
	const uint8_t* t2 = reinterpret_cast<const uint8_t*>(b.data());
	MscAlignTraceCount count;
	msc_align_trace_walk(dirs.data(), t1, t2, la, lb, start, count);
	std::vector<uint32_t> ops(count.n);
	MscAlignTraceWrite write{ops.data() + ops.size()};
	msc_align_trace_walk(dirs.data(), t1, t2, la, lb, start, write);
	if (write.end != ops.data()) { printf("the second walk wrote %zu of %zu runs\n", (size_t)(ops.data() + ops.size() - write.end), ops.size()); exit(1); }
	return ops;
}

}  // namespace

int main(int argc, char** argv) {
	if (argc != 2) { fprintf(stderr, "usage: align_trace_schedule_check pairs.txt\n"); return 2; }
	std::ifstream in(argv[1]);
	size_t n_seqs = 0, n_sets = 0, n_pairs = 0;
	in >> n_seqs >> n_sets >> n_pairs;
	std::vector<std::string> seqs(n_seqs);
	for (auto& s : seqs) in >> s;
	std::vector<int> par(4 * n_sets);
	for (auto& v : par) in >> v;
	std::vector<uint32_t> pr(2 * n_pairs);
	for (auto& v : pr) in >> v;
	std::vector<std::vector<uint32_t>> want(n_sets * n_pairs);
	for (auto& w : want) {
		size_t n = 0;
		in >> n;
		if (!in || n > (1u << 17)) break;
		w.resize(n);
		for (auto& v : w) in >> v;
	}
	if (!in || n_pairs == 0) { fprintf(stderr, "align_trace_schedule_check: %s is not a complete dump\n", argv[1]); return 2; }
	for (size_t s = 0; s < n_sets; s++) {
		const MscAlignParams P = msc_align_params(par[4 * s], par[4 * s + 1], par[4 * s + 2], par[4 * s + 3]);
		for (size_t p = 0; p < n_pairs; p++) {
			if (pr[2 * p] >= n_seqs || pr[2 * p + 1] >= n_seqs) { fprintf(stderr, "align_trace_schedule_check: pair %zu names a sequence past the list\n", p); return 2; }
			const std::vector<uint32_t> got = run_pair(seqs[pr[2 * p]], seqs[pr[2 * p + 1]], P), &w = want[s * n_pairs + p];
			if (got != w) {
				size_t k = 0;
				while (k < got.size() && k < w.size() && got[k] == w[k]) k++;
				printf("set %zu pair %zu (%zu x %zu): %zu runs, the dump holds %zu; the first difference is run %zu\n", s, p, seqs[pr[2 * p]].size(), seqs[pr[2 * p + 1]].size(), got.size(),
				       w.size(), k);
				return 1;
			}
		}
	}
	printf("%zu pairs under %zu parameter sets agree\n", n_pairs, n_sets);
	return 0;
}
