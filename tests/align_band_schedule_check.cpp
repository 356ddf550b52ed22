// align_band_schedule_check.cpp -- the schedule of k_align_band (meshclust2_amd/csrc/msc_align_band.hip) replayed serially on the host, over
// the band, the stripe windows, the carry ring, the per-lane step and the certificate of msc_align_band.h that the kernel itself compiles:
// stripes of 64 * C columns that visit only the rows of their window, lanes that start out of band below row 1, the overwrite of cells
// outside the band, the carry ring written by the last lane and read one row ahead by lane 0 of the next stripe, the one in-band cell above
// a window taken from the ring, the zero padding of the two sequences. Every pair runs under each number of columns a lane may keep
// (1, 2, 4), whatever the library would pick for its band.
//
//   align_band_schedule_check pairs.txt        (the dump of tests/align_band_util.py: write_dump)
//
// Prints the first case whose (score, length, matches, certified) differ from the dump's and exits 1; exits 0 when every case agrees. Built
// by tests/test_align_band_cpu.py with -fsanitize=address,undefined: an index outside the staged sequences or the ring ends the run.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "msc_align_band.h"

namespace {

struct Result {
	int32_t score, length, matches, certified;
};

template <int C>
Result run_pair(const std::string& a, const std::string& b, uint32_t w, const MscAlignParams& P) {
	constexpr uint32_t kStripe = kAlignLanes * C;
	const uint32_t la = (uint32_t)a.size(), lb = (uint32_t)b.size(), stripes = msc_align_band_stripes(la, kStripe);
	// the sequences as the workgroup's LDS holds them, byte for byte: exact sizes, so that the sanitizer sees every access past them
	std::vector<uint8_t> lds(msc_align_band_carry_at(la, lb, kStripe));
	uint8_t* s1 = lds.data();
	uint8_t* s2 = lds.data() + msc_align_band_seq2_at(la, kStripe) + kAlignSeqPad;
	for (uint32_t i = 0; i < stripes * kStripe; i++) s1[i] = i < la ? (uint8_t)a[i] : (uint8_t)0;
	for (uint32_t i = 0; i < lb + 2 * kAlignSeqPad; i++) s2[(int32_t)i - (int32_t)kAlignSeqPad] = i >= kAlignSeqPad && i < kAlignSeqPad + lb ? (uint8_t)b[i - kAlignSeqPad] : (uint8_t)0;
	std::vector<MscAlignTriple> carry(msc_align_band_carry_rows(la, lb, w, kStripe));          // (in LDS or in global memory: the same rows either way)
	std::vector<char> written(carry.size(), 0);                                                 // a row of the ring must have been written before it is read
	const MscAlignBand band = msc_align_band(la, lb, w);
	const uint32_t ring = msc_align_band_ring(la, lb, w, kStripe);
	const int32_t neg_inf = msc_align_neg_inf(la, lb, P);
	const MscAlignTriple deep = msc_align_deep();
	auto load = [&](uint32_t at) {
		if (!written.at(at)) { printf("ring row %u is read before it is written\n", at); exit(1); }
		return carry.at(at);
	};
	std::vector<MscAlignBandLane<C>> lanes(kAlignLanes);
	std::vector<MscAlignTriple> out(kAlignLanes), recv(kAlignLanes);
	for (uint32_t s = 0; s < stripes; s++) {
		const uint32_t c0 = s * kStripe + 1;
		const MscAlignWindow win = msc_align_band_window(band, la, lb, c0, kStripe);
		if (win.r1 < win.r0 || win.r1 - win.r0 + 1 > ring) { printf("stripe %u: a window of rows %u .. %u over a ring of %u\n", s, win.r0, win.r1, ring); exit(1); }
		const uint32_t steps = win.r1 - win.r0 + kAlignLanes;
		uint32_t rd = win.r0 % ring;
		const MscAlignTriple corner = s && win.r0 > 1 ? load(rd ? rd - 1 : ring - 1) : deep;
		for (uint32_t lane = 0; lane < (uint32_t)kAlignLanes; lane++) {
			const uint32_t first = c0 + lane * C;
			uint32_t bytes = 0;
			for (int c = 0; c < C; c++) bytes |= (uint32_t)s1[first - 1 + c] << (8 * c);
			msc_align_band_lane_init(lanes[lane], band, first, bytes, win.r0, lane == 0, corner, neg_inf, P);
			out[lane] = lanes[lane].col[C - 1];
		}
		uint32_t wr = rd;
		MscAlignTriple next = msc_align_band_left(win, s == 0, win.r0, (int32_t)win.r0 <= win.read_hi && s ? load(rd) : deep, neg_inf, P);
		for (uint32_t t = 0; t < steps; t++) {
			for (uint32_t lane = kAlignLanes - 1; lane >= 1; lane--) recv[lane] = out[lane - 1];          // the wave shift
			recv[0] = next;
			const uint32_t ahead = win.r0 + t + 1;
			rd = rd + 1 == ring ? 0 : rd + 1;
			next = msc_align_band_left(win, s == 0, ahead, (int32_t)ahead <= win.read_hi && s ? load(rd) : deep, neg_inf, P);
			for (uint32_t lane = 0; lane < (uint32_t)kAlignLanes; lane++) {
				const int32_t row = (int32_t)(win.r0 + t) - (int32_t)lane;
				const uint32_t byte = s2[row - 1];
				if (row >= (int32_t)win.r0 && row <= (int32_t)win.r1) {
					msc_align_band_lane_step(lanes[lane], band, c0 + lane * C, (uint32_t)row, recv[lane], byte, P);
					if (lane == (uint32_t)kAlignLanes - 1 && s + 1 < stripes) {
						carry.at(wr) = lanes[lane].col[C - 1];
						written.at(wr) = 1;
						wr = wr + 1 == ring ? 0 : wr + 1;
					}
				}
				out[lane] = lanes[lane].col[C - 1];
			}
		}
	}
	const uint32_t at = (la - 1) % kStripe;
	const MscAlignState r = msc_align_final(lanes[at / C].col[at % C]);
	return Result{r.s, (int32_t)(r.w >> 16), (int32_t)(r.w & 0xffffu), msc_align_band_certified(la, lb, w, P, r.s) ? 1 : 0};
}

}  // namespace

int main(int argc, char** argv) {
	if (argc != 2) { fprintf(stderr, "usage: align_band_schedule_check pairs.txt\n"); return 2; }
	std::ifstream in(argv[1]);
	size_t n_seqs = 0, n_sets = 0, n_pairs = 0, n_bands = 0;
	in >> n_seqs >> n_sets >> n_pairs >> n_bands;
	std::vector<std::string> seqs(n_seqs);
	for (auto& s : seqs) in >> s;
	std::vector<int> par(4 * n_sets);
	for (auto& v : par) in >> v;
	std::vector<uint32_t> pr(2 * n_pairs);
	for (auto& v : pr) in >> v;
	std::vector<uint32_t> bands(n_bands);
	for (auto& v : bands) in >> v;
	std::vector<Result> want(n_sets * n_bands * n_pairs);
	for (auto& w : want) in >> w.score >> w.length >> w.matches >> w.certified;
	if (!in || n_pairs == 0 || n_bands == 0) { fprintf(stderr, "align_band_schedule_check: %s is not a complete dump\n", argv[1]); return 2; }
	size_t certified = 0;
	for (size_t s = 0; s < n_sets; s++) {
		const MscAlignParams P = msc_align_params(par[4 * s], par[4 * s + 1], par[4 * s + 2], par[4 * s + 3]);
		for (size_t k = 0; k < n_bands; k++)
			for (size_t p = 0; p < n_pairs; p++) {
				if (pr[2 * p] >= n_seqs || pr[2 * p + 1] >= n_seqs) { fprintf(stderr, "align_band_schedule_check: pair %zu names a sequence past the list\n", p); return 2; }
				const std::string &a = seqs[pr[2 * p]], &b = seqs[pr[2 * p + 1]];
				const Result& w = want[(s * n_bands + k) * n_pairs + p];
				const Result got[3] = {run_pair<1>(a, b, bands[k], P), run_pair<2>(a, b, bands[k], P), run_pair<4>(a, b, bands[k], P)};
				for (int v = 0; v < 3; v++)
					if (got[v].score != w.score || got[v].length != w.length || got[v].matches != w.matches || got[v].certified != w.certified) {
						printf("set %zu band %u pair %zu (%zu x %zu), %d columns a lane: got %d %d %d %d, the dump holds %d %d %d %d\n", s, bands[k], p, a.size(), b.size(), 1 << v,
						       got[v].score, got[v].length, got[v].matches, got[v].certified, w.score, w.length, w.matches, w.certified);
						return 1;
					}
				certified += (size_t)w.certified;
			}
	}
	printf("%zu pairs at %zu half-widths under %zu parameter sets agree, %zu certified\n", n_pairs, n_bands, n_sets, certified);
	return 0;
}
