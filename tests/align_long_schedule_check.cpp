// align_long_schedule_check.cpp -- the schedule of k_align_tiles (meshclust2_amd/csrc/msc_align_long.hip) replayed on the host in launch order,
// over the tiles, the borders and a lane's start of msc_align_long.h and the band, the per-lane step and the certificate of msc_align_band.h
// that the kernel itself compiles, all over wide states. The borders of a pair are one array laid out as on the device (the column border,
// then a row border per stripe), filled with a poison pattern before the first launch; every entry also remembers the launch that wrote it,
// and a read of an entry that nobody wrote, or that a tile of the SAME launch wrote, ends the run -- as does a second write to an entry
// within one launch. The tiles of a launch run from the last stripe to the first in every other launch: their order must not matter.
//
//   align_long_schedule_check pairs.txt --rows 64,100,1024 --bands full,1,64,300 [--nest] [--must-certify]
//
// pairs.txt is the dump of tests/align_util.py: write_dump with the FULL alignment's integers. Every pair runs at every tile height and
// half-width, under every parameter set of the dump. A full-grid result, and a banded one whose certificate holds, must equal the dump's
// integers. With --nest every result -- uncertified ones too: the band defines them -- must equal a plain loop nest over the rows of the
// grid, written below from the definition in DESIGN.md 4.6f and from nothing of the schedule. With --must-certify every banded result must
// carry its certificate. Prints the first disagreement and exits 1; exits 0 when everything agrees. tests/test_align_long_cpu.py builds it
// with -fsanitize=address,undefined (the short fixture, with --nest) and plainly (the long fixture).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "msc_align_long.h"

namespace {

struct Result {
	int32_t score, length, matches, certified;
};
bool same(const Result& a, const Result& b) { return a.score == b.score && a.length == b.length && a.matches == b.matches && a.certified == b.certified; }

constexpr uint32_t kNever = 0xffffffffu;

// a range of a pair's borders, with the checks
struct Border {
	std::vector<MscAlignWideTriple>* v;
	std::vector<uint32_t>* stamp;          // the launch that wrote the entry
	size_t base, size;
	uint32_t launch;
	const MscAlignWideTriple& operator[](size_t i) const {
		if (i >= size) { printf("launch %u: entry %zu of a border of %zu is read\n", launch, i, size); exit(1); }
		const uint32_t s = stamp->at(base + i);
		if (s == kNever) { printf("launch %u: entry %zu of the border at %zu is read, nobody wrote it\n", launch, i, base); exit(1); }
		if (s >= launch) { printf("launch %u: entry %zu of the border at %zu is read, a tile of launch %u wrote it\n", launch, i, base, s); exit(1); }
		return v->at(base + i);
	}
	void write(size_t i, const MscAlignWideTriple& t) const {
		if (i >= size) { printf("launch %u: entry %zu of a border of %zu is written\n", launch, i, size); exit(1); }
		if (stamp->at(base + i) == launch) { printf("launch %u: entry %zu of the border at %zu is written twice\n", launch, i, base); exit(1); }
		v->at(base + i) = t;
		stamp->at(base + i) = launch;
	}
};

struct Pair {
	const std::string *a, *b;
	uint32_t w;
	MscAlignParams P;
	uint32_t H;
	std::vector<MscAlignWideTriple> borders;
	std::vector<uint32_t> stamp;
	Result result;
	bool reported;
};

// one tile: what a wave of k_align_tiles does
void run_tile(Pair& pr, uint32_t stripe, uint32_t block, uint32_t launch) {
	const uint32_t la = (uint32_t)pr.a->size(), lb = (uint32_t)pr.b->size(), stripes = msc_align_stripes(la), H = pr.H;
	const MscAlignParams& P = pr.P;
	const MscAlignBand band = msc_align_long_band(la, lb, pr.w);
	const MscAlignTile tile = msc_align_tile(band, la, lb, stripe, block, H);
	if (tile.bot < tile.top || tile.bot - tile.top + 1 > H) { printf("tile (%u, %u): rows %u .. %u\n", stripe, block, tile.top, tile.bot); exit(1); }
	const uint32_t rows = tile.bot - tile.top + 1;
	std::vector<uint8_t> lds(rows + 2 * kAlignSeqPad);          // exact size, so that the sanitizer sees every access past it
	for (uint32_t i = 0; i < rows + 2 * kAlignSeqPad; i++) lds[i] = i >= kAlignSeqPad && i < kAlignSeqPad + rows ? (uint8_t)(*pr.b)[(tile.top - 1) + (i - kAlignSeqPad)] : (uint8_t)0;
	const Border col_border{&pr.borders, &pr.stamp, 0, (size_t)msc_align_long_row_at(lb), launch};
	const Border row_border{&pr.borders, &pr.stamp, (size_t)(msc_align_long_row_at(lb) + (uint64_t)stripe * kAlignRowBorder), kAlignRowBorder, launch};
	const int32_t neg_inf = msc_align_neg_inf(la, lb, P);
	const MscAlignWideTriple deep = msc_align_wide_deep();
	std::vector<MscAlignWideLane> lanes(kAlignLanes);
	std::vector<MscAlignWideTriple> out(kAlignLanes), recv(kAlignLanes);
	for (uint32_t lane = 0; lane < (uint32_t)kAlignLanes; lane++) {
		const uint32_t first = tile.c0 + lane * kAlignCols;
		uint32_t bytes = 0;
		for (int c = 0; c < kAlignCols; c++) if (first - 1 + c < la) bytes |= (uint32_t)(uint8_t)(*pr.a)[first - 1 + c] << (8 * c);
		msc_align_tile_start(lanes[lane], band, tile, lane, bytes, col_border, row_border, neg_inf, P);
		out[lane] = lanes[lane].col[kAlignCols - 1];
	}
	const bool writes = stripe + 1 < stripes;
	const uint32_t steps = rows + kAlignLanes - 1;
	MscAlignWideTriple next = msc_align_tile_left(tile, tile.top, col_border, neg_inf, P);
	for (uint32_t t = 0; t < steps; t++) {
		for (uint32_t lane = kAlignLanes - 1; lane >= 1; lane--) recv[lane] = out[lane - 1];          // the wave shift
		recv[0] = next;
		const uint32_t ahead = tile.top + t + 1;
		next = ahead <= tile.bot ? msc_align_tile_left(tile, ahead, col_border, neg_inf, P) : deep;
		for (uint32_t lane = 0; lane < (uint32_t)kAlignLanes; lane++) {
			const int32_t row = (int32_t)(tile.top + t) - (int32_t)lane;
			const uint32_t byte = lds.at((size_t)((int32_t)(kAlignSeqPad + t) - (int32_t)lane));
			if (row >= (int32_t)tile.top && row <= (int32_t)tile.bot) {
				msc_align_band_lane_step(lanes[lane], band, tile.c0 + lane * kAlignCols, (uint32_t)row, recv[lane], byte, P);
				if (lane == (uint32_t)kAlignLanes - 1 && writes) col_border.write((size_t)row, lanes[lane].col[kAlignCols - 1]);
			}
			out[lane] = lanes[lane].col[kAlignCols - 1];
		}
	}
	if (tile.bot < tile.win.r1) {
		for (uint32_t lane = 0; lane < (uint32_t)kAlignLanes; lane++)
			for (int c = 0; c < kAlignCols; c++) row_border.write(1 + lane * kAlignCols + c, lanes[lane].col[c]);
		row_border.write(0, lanes[0].prev);
	}
	if (stripe + 1 == stripes && tile.bot == lb) {
		const uint32_t at = (la - 1) % kAlignStripe;
		const MscAlignStateT<MscAlignWide> r = msc_align_final(lanes[at / kAlignCols].col[at % kAlignCols]);
		if (pr.reported) { printf("two tiles report the pair's result\n"); exit(1); }
		pr.reported = true;
		pr.result = Result{r.s, (int32_t)MscAlignCount<MscAlignWide>::length(r.w), (int32_t)MscAlignCount<MscAlignWide>::matches(r.w), msc_align_band_certified(la, lb, pr.w, P, r.s) ? 1 : 0};
	}
}

Result run_pair(const std::string& a, const std::string& b, uint32_t w, uint32_t H, const MscAlignParams& P) {
	const uint32_t la = (uint32_t)a.size(), lb = (uint32_t)b.size(), stripes = msc_align_stripes(la);
	Pair pr{&a, &b, w, P, H, {}, {}, Result{0, 0, 0, 0}, false};
	MscAlignWideTriple poison;
	poison.m.s = poison.l.s = poison.u.s = 2000000000;          // wins every comparison it takes part in
	poison.m.w = poison.l.w = poison.u.w = MscAlignWide{0xddddddddu, 0xddddddddu};
	pr.borders.assign((size_t)msc_align_long_borders(la, lb), poison);
	pr.stamp.assign(pr.borders.size(), kNever);
	const MscAlignBand band = msc_align_long_band(la, lb, w);
	const uint32_t launches = stripes + (lb - 1) / H;
	size_t tiles = 0;
	for (uint32_t d = 0; d < launches; d++)
		for (uint32_t k = 0; k < stripes; k++) {
			const uint32_t s = d & 1 ? stripes - 1 - k : k;
			if (s > d) continue;
			const MscAlignWindow win = msc_align_band_window(band, la, lb, s * kAlignStripe + 1, kAlignStripe);
			if (win.r1 < win.r0) { printf("stripe %u: a window of rows %u .. %u\n", s, win.r0, win.r1); exit(1); }
			const uint32_t b = d - s;
			if (b < msc_align_first_block(win, H) || b > msc_align_last_block(win, H)) continue;
			run_tile(pr, s, b, d);
			tiles++;
		}
	if (!pr.reported) { printf("no tile of %zu reported the pair's result\n", tiles); exit(1); }
	return pr.result;
}

// ---------------------------------------------------------------------------------------- the definition, row by row
// three states a cell, each a score, a length and a count of identical columns; every state of a cell outside the
// band lo <= i - j <= hi, boundary cells included, is (-2^30, 0, 0)
struct St {
	int64_t s;
	uint32_t len, cnt;
};
struct Cell {
	St m, l, u;
};
Result nest(const std::string& a, const std::string& b, uint32_t w, int match, int mismatch, int open, int cont) {
	const int64_t la = (int64_t)a.size(), lb = (int64_t)b.size(), d = la - lb, ww = w > 4000000u ? 4000000 : (int64_t)w;
	const int64_t lo = (d < 0 ? d : 0) - ww, hi = (d > 0 ? d : 0) + ww, deep = -(1ll << 30);
	int64_t ninf = mismatch * (la < lb ? la : lb) - 1;
	if (d != 0) ninf += -open - (d < 0 ? -d : d) * cont;
	const St out_of_band{deep, 0, 0};
	auto gap = [&](const St& from_match, const St& from_gap) {
		const int64_t x = from_match.s - (open + cont), y = from_gap.s - cont;
		return x >= y ? St{x, from_match.len + 1, from_match.cnt} : St{y, from_gap.len + 1, from_gap.cnt};
	};
	auto best = [](const Cell& c) { return c.m.s >= c.l.s ? (c.m.s >= c.u.s ? c.m : c.u) : (c.l.s >= c.u.s ? c.l : c.u); };          // match, then lower, then upper
	std::vector<Cell> above((size_t)la + 1), row((size_t)la + 1);
	for (int64_t j = 0; j <= lb; j++) {
		for (int64_t i = 0; i <= la; i++) {
			Cell& c = row[(size_t)i];
			if (i - j < lo || i - j > hi) c = Cell{out_of_band, out_of_band, out_of_band};
			else if (j == 0 && i == 0) c = Cell{St{0, 0, 0}, St{ninf, 0, 0}, St{-open, 0, 0}};
			else if (j == 0) c = Cell{St{ninf, (uint32_t)i, 0}, St{-open - i * cont, (uint32_t)i, 0}, St{ninf, (uint32_t)i, 0}};
			else if (i == 0) c = Cell{St{ninf, (uint32_t)j, 0}, St{ninf, (uint32_t)j, 0}, St{-open - j * cont, (uint32_t)j, 0}};
			else {
				const bool eq = a[(size_t)i - 1] == b[(size_t)j - 1];
				const int64_t add = eq ? match : mismatch;
				const St from = best(above[(size_t)i - 1]);
				c.m = St{from.s + add, from.len + 1, from.cnt + (add == match ? 1u : 0u)};
				c.l = gap(row[(size_t)i - 1].m, row[(size_t)i - 1].l);
				c.u = gap(above[(size_t)i].m, above[(size_t)i].u);
			}
		}
		above.swap(row);
	}
	const St r = best(above[(size_t)la]);
	const MscAlignParams P = msc_align_params(match, mismatch, open, cont);
	return Result{(int32_t)r.s, (int32_t)r.len, (int32_t)r.cnt, msc_align_band_certified((uint32_t)la, (uint32_t)lb, w, P, (int32_t)r.s) ? 1 : 0};
}

std::vector<uint32_t> numbers(const char* list) {
	std::vector<uint32_t> v;
	for (const char* p = list; *p;) {
		if (!strncmp(p, "full", 4)) { v.push_back(kAlignBandNone); p += 4; }
		else { char* end; v.push_back((uint32_t)strtoul(p, &end, 10)); if (end == p) return {}; p = end; }
		if (*p == ',') p++;
	}
	return v;
}

}  // namespace

int main(int argc, char** argv) {
	std::vector<uint32_t> heights, bands;
	bool with_nest = false, must_certify = false;
	for (int i = 2; i < argc; i++) {
		if (!strcmp(argv[i], "--rows") && i + 1 < argc) heights = numbers(argv[++i]);
		else if (!strcmp(argv[i], "--bands") && i + 1 < argc) bands = numbers(argv[++i]);
		else if (!strcmp(argv[i], "--nest")) with_nest = true;
		else if (!strcmp(argv[i], "--must-certify")) must_certify = true;
		else argc = 0;
	}
	if (argc < 2 || heights.empty() || bands.empty()) { fprintf(stderr, "usage: align_long_schedule_check pairs.txt --rows H,... --bands full|W,... [--nest] [--must-certify]\n"); return 2; }
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
	for (auto& w : want) { in >> w.score >> w.length >> w.matches; w.certified = 1; }
	if (!in || n_pairs == 0) { fprintf(stderr, "align_long_schedule_check: %s is not a complete dump\n", argv[1]); return 2; }
	size_t runs = 0, certified = 0;
	for (size_t s = 0; s < n_sets; s++) {
		const int* q = &par[4 * s];
		const MscAlignParams P = msc_align_params(q[0], q[1], q[2], q[3]);
		for (size_t p = 0; p < n_pairs; p++) {
			if (pr[2 * p] >= n_seqs || pr[2 * p + 1] >= n_seqs) { fprintf(stderr, "align_long_schedule_check: pair %zu names a sequence past the list\n", p); return 2; }
			const std::string &a = seqs[pr[2 * p]], &b = seqs[pr[2 * p + 1]];
			for (uint32_t w : bands) {
				const Result by_definition = with_nest ? nest(a, b, w, q[0], q[1], q[2], q[3]) : Result{0, 0, 0, 0};
				for (uint32_t H : heights) {
					const Result got = run_pair(a, b, w, H, P);
					const char* against = nullptr;
					const Result* other = nullptr;
					if (with_nest && !same(got, by_definition)) { against = "the loop nest gives"; other = &by_definition; }
					else if (got.certified && !same(got, want[s * n_pairs + p])) { against = "the dump holds"; other = &want[s * n_pairs + p]; }
					else if ((must_certify || w == kAlignBandNone) && !got.certified) { against = "a certificate was due:"; other = &want[s * n_pairs + p]; }
					if (against) {
						printf("set %zu pair %zu (%zu x %zu), half-width %u, %u rows a tile: got %d %d %d %d, %s %d %d %d %d\n", s, p, a.size(), b.size(), w, H, got.score, got.length,
						       got.matches, got.certified, against, other->score, other->length, other->matches, other->certified);
						return 1;
					}
					runs++;
					certified += (size_t)got.certified;
				}
			}
		}
	}
	printf("%zu pairs under %zu parameter sets: %zu runs agree, %zu certified\n", n_pairs, n_sets, runs, certified);
	return 0;
}
