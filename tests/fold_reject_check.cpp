// fold_reject_check.cpp -- stand-alone check of the folded block's integer cut (meshclust2_amd/csrc/msc_fold_reject.h; built and run by
// tests/test_fold_reject_cpu.py with -fsanitize=address,undefined). Two modes:
//
//   fold_reject_check soundness <models> <pairs per model> <weights file> ...
//       random models over the nine `fast` statistics, and the classification block of every weights file given: random launches (a query,
//       a handful of candidates, the ranges of those), the cut T(q) of the header, and for every candidate pairs drawn INSIDE what the cut
//       claims to cover -- U <= T(q), the sums S and D anywhere up to what the fold and the lists allow for that U, the distance anywhere up to
//       the two moments, the ends most of the time. A pair whose FP64 evaluation (the formulas of predict/Feature.cpp, written out below) is
//       close is a failure.
//   fold_reject_check sample <sequences> <weights file> <k> <dtype> <order> <family> <query stride> [<out>]
//       the sequences of a file (one per line, ACGT): histograms, folded F = 16 presence bits, lists of large bins and rank moments on the CPU
//       as the mirrors hold them; T(q) for every stride-th sequence against the ranges of all of them; the share of UNRELATED pairs (another
//       family) with U = P1' + P2' <= T(q); every such pair evaluated in FP64 from its true reductions. <out>: int32 T per query, then a byte per
//       (query, candidate): 1 when the cut rejects the pair.
// Exit status 0 = every check held.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../meshclust2_amd/csrc/msc_fold_reject.h"

typedef unsigned long long ull;
static const int kMaxSingles = 16, kMaxCombos = 8;
static const uint64_t kFast[9] = {MSC_RJ_MANHATTAN, MSC_RJ_EUCLIDEAN, MSC_RJ_NORMALIZED_VECTORS, MSC_RJ_PEARSON_COEFF, MSC_RJ_INTERSECTION,
                                  MSC_RJ_EMD,       MSC_RJ_LENGTHD,   MSC_RJ_KULCZYNSKI2,        MSC_RJ_SIMRATIO};

// ---------------------------------------------------------------- the model: FP64 as the weights file has it, and its f32 image
struct Model {
	int n_singles = 0, n_combos = 0;
	uint64_t single_flag[kMaxSingles];
	double mins[kMaxSingles], maxs[kMaxSingles];
	int is_sim[kMaxSingles];
	int combo_kind[kMaxCombos], combo_n[kMaxCombos], combo_idx[kMaxCombos][2];
	double weights[kMaxCombos + 1];
	int screen_ok = 0;
	float s_min[kMaxSingles], s_inv[kMaxSingles], s_w[kMaxCombos + 1];
};

static int is_sim_of(uint64_t f) {          // Feature<T>::feat_is_sim, predict/Feature.cpp:549-663
	return f == MSC_RJ_NORMALIZED_VECTORS || f == MSC_RJ_PEARSON_COEFF || f == MSC_RJ_INTERSECTION || f == MSC_RJ_KULCZYNSKI2 || f == MSC_RJ_SIMRATIO;
}
static int index_of(const Model& m, uint64_t f) {
	for (int i = 0; i < m.n_singles; i++) if (m.single_flag[i] == f) return i;
	return -1;
}
// Feature::add_feature (predict/Feature.cpp:102-128): the singles in ascending-bit order of first appearance
static bool add_combo(Model& m, int kind, uint64_t flags, double w) {
	const int c = m.n_combos;
	if (c >= kMaxCombos) return false;
	int n = 0;
	for (uint64_t f = 1; f != 0 && f <= flags; f <<= 1) {
		if (!(flags & f)) continue;
		if (index_of(m, f) < 0) {
			if (m.n_singles >= kMaxSingles) return false;
			m.single_flag[m.n_singles] = f; m.is_sim[m.n_singles] = is_sim_of(f); m.mins[m.n_singles] = 0; m.maxs[m.n_singles] = 1;
			m.n_singles++;
		}
		if (n >= 2) return false;
		m.combo_idx[c][n++] = index_of(m, f);
	}
	if (n == 0 || (n == 1 && (kind == MSC_RJ_XY2 || kind == MSC_RJ_X2Y))) return false;
	if (n == 1) m.combo_idx[c][1] = m.combo_idx[c][0];
	m.combo_kind[c] = kind; m.combo_n[c] = n; m.weights[c + 1] = w;
	m.n_combos++;
	return true;
}
static void f32_image(Model& m) {          // model_screen_image of msc_api.hip
	m.screen_ok = 0;
	if (m.n_singles < 1 || m.n_combos < 1) return;
	for (int i = 0; i < m.n_singles; i++) {
		bool fast = false;
		for (uint64_t f : kFast) fast = fast || f == m.single_flag[i];
		if (!fast) return;
		const double range = m.maxs[i] - m.mins[i];
		const float mn = (float)m.mins[i], inv = (float)(1.0 / range);
		if (!(range != 0.0) || !std::isfinite(mn) || !std::isfinite(inv) || inv == 0.f) return;
		m.s_min[i] = mn; m.s_inv[i] = inv;
	}
	for (int c = 0; c <= m.n_combos; c++) { m.s_w[c] = (float)m.weights[c]; if (!std::isfinite(m.s_w[c])) return; }
	m.screen_ok = 1;
}
// the classification block of a weights file (Predictor::read_from, predict/Predictor.cpp:125-185): `n_combos: n`, the intercept, n lines of
// (kind, flags, weight); `n_singles: n`, n lines of (flag, min, max)
static bool parse_weights(const char* path, Model& m, int* k_out) {
	std::ifstream in(path);
	if (!in) return false;
	std::string tok;
	m = Model();
	while (in >> tok) {
		if (tok == "k:") in >> *k_out;
		if (tok == "n_combos:") break;
	}
	int nc = 0, ns = 0;
	if (!(in >> nc >> m.weights[0])) return false;
	for (int c = 0; c < nc; c++) {
		int kind; ull flags; double w;
		if (!(in >> kind >> flags >> w) || !add_combo(m, kind, flags, w)) return false;
	}
	if (!(in >> tok >> ns) || tok != "n_singles:") return false;
	for (int i = 0; i < ns; i++) {
		ull f; double mn, mx;
		if (!(in >> f >> mn >> mx)) return false;
		const int idx = index_of(m, f);
		if (idx < 0) return false;
		m.mins[idx] = mn; m.maxs[idx] = mx;
	}
	f32_image(m);
	return true;
}

// ---------------------------------------------------------------- the FP64 evaluation of a pair from its integer reductions
struct Side { uint64_t mag, len, sum, sq; };
struct Totals { uint64_t manh, dot, emd; };

// a = the first argument of the reference call, b = the second (predict/Feature.cpp, by the statistic's lines)
static double raw_stat(uint64_t flag, const Totals& t, const Side& a, const Side& b, uint64_t nbins, int dtype) {
	const double N = (double)nbins;
	switch (flag) {
	case MSC_RJ_MANHATTAN: return (double)(int32_t)(uint32_t)t.manh;                                      // `int sum`, :864-870
	case MSC_RJ_EUCLIDEAN: return sqrt((double)(a.sq + b.sq - 2 * t.dot));                                // :1118-1123
	case MSC_RJ_NORMALIZED_VECTORS: return (double)t.dot / sqrt((double)(a.sq * b.sq));                   // :1176-1183
	case MSC_RJ_PEARSON_COEFF: {                                                                          // :800-810
		const double dap = (double)a.mag / N, daq = (double)b.mag / N;
		const double np = (double)a.sq - 2.0 * dap * (double)a.sum + N * dap * dap;
		const double nq = (double)b.sq - 2.0 * daq * (double)b.sum + N * daq * daq;
		const double dt = (double)t.dot - daq * (double)a.sum - dap * (double)b.sum + N * dap * daq;
		return dt / sqrt(np * nq);
	}
	case MSC_RJ_INTERSECTION: return (double)(2 * ((a.sum + b.sum - t.manh) >> 1)) / (double)(a.mag + b.mag);      // :769-776
	case MSC_RJ_EMD: return (double)t.emd;                                                                // :1510-1517
	case MSC_RJ_LENGTHD: return (double)(a.len > b.len ? a.len - b.len : b.len - a.len);                  // :878-886
	case MSC_RJ_KULCZYNSKI2: {                                                                            // :686-694
		const double ap = (double)a.mag / N, aq = (double)b.mag / N;
		return N * (ap + aq) / (2 * ap * aq) * (double)((a.sum + b.sum - t.manh) >> 1);
	}
	case MSC_RJ_SIMRATIO: {                                                                               // :834-840
		uint64_t norm2 = a.sq + b.sq - 2 * t.dot;
		if (dtype == 32) {          // `intmax_t diff = p - q` wraps mod 2^32 for 32-bit bins before widening: every bin with p < q adds (q - p)^2 - 2^33 (q - p)
			const int64_t sdiff = (int64_t)a.sum - (int64_t)b.sum;
			norm2 -= (uint64_t)(((int64_t)t.manh - sdiff) >> 1) << 33;
		}
		return (double)t.dot / ((double)t.dot + sqrt((double)norm2));
	}
	default: return NAN;
	}
}

// Feature::normalize_cache (:137-154), Feature::operator() (Feature.h:205-239), Trainer::classify (cluster/Trainer.cpp:112-120) -> the sum, and
// whether the pair is close (GLM::logistic, predict/GLM.cpp:26-29)
static double weighted_sum(const Model& m, const Totals& t, const Side& a, const Side& b, uint64_t nbins, int dtype, bool* close) {
	double v[kMaxSingles];
	for (int i = 0; i < m.n_singles; i++) {
		const double val = (raw_stat(m.single_flag[i], t, a, b, nbins, dtype) - m.mins[i]) / (m.maxs[i] - m.mins[i]);
		v[i] = m.is_sim[i] ? val : 1 - val;
	}
	double sum = m.weights[0];
	for (int c = 0; c < m.n_combos; c++) {
		const int i0 = m.combo_idx[c][0], i1 = m.combo_idx[c][1], n = m.combo_n[c];
		double d;
		switch (m.combo_kind[c]) {
		case MSC_RJ_XY: d = 1; d *= v[i0]; if (n == 2) d *= v[i1]; break;
		case MSC_RJ_X2Y2: d = 1; d *= v[i0] * v[i0]; if (n == 2) d *= v[i1] * v[i1]; break;
		case MSC_RJ_XY2: d = v[i0] * v[i1] * v[i1]; break;
		default: d = v[i0] * v[i0] * v[i1]; break;
		}
		sum += m.weights[c + 1] * d;
	}
	*close = std::round(1.0 / (1 + exp(-sum))) > 0;
	return sum;
}

// ---------------------------------------------------------------- random numbers (SplitMix64)
struct Rng {
	uint64_t s;
	uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
	double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
	uint64_t below(uint64_t n) { return n ? next() % n : 0; }
	uint64_t in(uint64_t lo, uint64_t hi) { return lo + below(hi - lo + 1); }
	// an end most of the time, else anywhere in [0, hi]
	uint64_t ends(uint64_t hi) { const uint64_t r = below(8); return r < 3 ? 0 : r < 6 ? hi : below(hi + 1); }
};

// ---------------------------------------------------------------- soundness on drawn pairs
// One slot of a launch as the mirrors describe it: a sequence of `len` bases with a few large bins
struct Slot {
	Side s;
	uint64_t rk_dev, g;          // the second rank moment; the sum of (e - 1) over the list of large bins
	uint32_t x, e_max;
};

static Slot draw_slot(Rng& r, int k, uint64_t nbins, uint64_t len, bool stale_mag) {
	Slot o;
	const uint64_t n_kmers = len >= (uint64_t)k ? len - k + 1 : 0;
	uint64_t left = n_kmers, sq = nbins;
	o.g = 0; o.e_max = 1;
	const uint32_t n_large = r.below(4) == 0 ? (uint32_t)r.below(4) : 0;
	for (uint32_t i = 0; i < n_large && left >= 2; i++) {
		uint64_t e = 2 + (r.below(4) == 0 ? r.below(400) : r.below(4));
		if (e > left) e = left;
		if (e < 2) break;
		left -= e; sq += e * e + 2 * e; o.g += e - 1;
		if (e > o.e_max) o.e_max = (uint32_t)e;
	}
	sq += 3 * left;          // the k-mers counted once: bins of 2
	o.s.len = len; o.s.sum = nbins + n_kmers; o.s.sq = sq;
	o.s.mag = o.s.sum;
	if (stale_mag) o.s.mag = o.s.sum + r.below(41) - (o.s.sum > 20 ? 20 : 0);          // (DivergencePoint::set leaves mag stale)
	o.x = (uint32_t)r.below(n_kmers / 8 + 1);
	o.rk_dev = r.below(n_kmers * nbins / 4 + 1);
	return o;
}

static void widen(MscRejectRanges& c, const Slot& s, bool first) {
	auto mm = [&](uint64_t& lo, uint64_t& hi, uint64_t v) { if (first || v < lo) lo = v; if (first || v > hi) hi = v; };
	mm(c.mag_lo, c.mag_hi, s.s.mag); mm(c.len_lo, c.len_hi, s.s.len); mm(c.sum_lo, c.sum_hi, s.s.sum); mm(c.sq_lo, c.sq_hi, s.s.sq);
	if (first || s.rk_dev > c.rk_dev_hi) c.rk_dev_hi = s.rk_dev;
	if (first || s.g > c.g_hi) c.g_hi = s.g;
}
static MscRejectQuery query_of(const Slot& s) { return MscRejectQuery{s.s.mag, s.s.len, s.s.sum, s.s.sq, s.rk_dev, s.x, s.e_max}; }

// the reductions of a pair from its two sums
static Totals totals_of(const Slot& q, const Slot& c, uint64_t nbins, uint64_t S, uint64_t D, uint64_t emd) {
	const uint64_t ex_c = c.s.sum - nbins, ex_q = q.s.sum - nbins;
	Totals t;
	t.manh = ex_c + ex_q - 2 * S;
	t.dot = nbins + ex_c + ex_q + D;
	const uint64_t top = (c.s.sq + q.s.sq) >> 1;          // sum c_i q_i cannot pass it
	if (t.dot > top) t.dot = top;
	t.emd = emd;
	return t;
}

// a model over the nine statistics whose normalisation spans an unrelated and an identical pair of ~len bases, as a trained one does
static Model random_model(Rng& r, int k, uint64_t nbins, int dtype, uint64_t len) {
	Model m;
	for (;;) {
		m = Model();
		const int nc = 1 + (int)r.below(4);
		bool ok = true;
		for (int c = 0; c < nc && ok; c++) {
			uint64_t flags = kFast[r.below(9)];
			if (r.below(3)) flags |= kFast[r.below(9)];
			const int two = (flags & (flags - 1)) != 0;
			const int kind = two ? (int)r.below(4) : (r.below(2) ? MSC_RJ_XY : MSC_RJ_X2Y2);
			ok = add_combo(m, kind, flags, (r.unit() - 0.4) * 8.0);
		}
		if (ok) break;
	}
	Slot a = draw_slot(r, k, nbins, len, false), b = draw_slot(r, k, nbins, len + r.below(len / 50 + 1), false);
	const uint64_t ex = std::min(a.s.sum, b.s.sum) - nbins;
	const Totals far = totals_of(a, b, nbins, ex / 200, ex / 200, a.rk_dev + b.rk_dev), near = totals_of(a, a, nbins, a.s.sum - nbins, a.s.sq + nbins - 2 * a.s.sum, 0);
	double s_far;
	for (int i = 0; i < m.n_singles; i++) {
		double v0 = raw_stat(m.single_flag[i], far, a.s, b.s, nbins, dtype), v1 = raw_stat(m.single_flag[i], near, a.s, a.s, nbins, dtype);
		if (m.single_flag[i] == MSC_RJ_LENGTHD) v1 = (double)(len / 4 + 1);
		if (!(v0 == v0) || !(v1 == v1) || v0 == v1) { v0 = 0; v1 = 1; }
		double lo = std::min(v0, v1), hi = std::max(v0, v1);
		const double span = hi - lo;
		lo -= span * 0.3 * r.unit(); hi += span * 0.3 * r.unit();
		m.mins[i] = lo; m.maxs[i] = hi;
	}
	// the intercept: the unrelated pair's sum lands a little -- or well -- below 0, so that cuts of every rung and none come out
	m.weights[0] = 0;
	bool close;
	s_far = weighted_sum(m, far, a.s, b.s, nbins, dtype, &close);
	static const double below[6] = {0.01, 0.05, 0.2, 0.6, 1.5, 4.0};
	if (s_far == s_far) m.weights[0] = -s_far - below[r.below(6)];
	f32_image(m);
	return m;
}

static const ull kMaxLaunches = 100000;
struct Tally { ull launches = 0, no_cut = 0, pairs = 0, close_uncovered = 0, bad = 0; ull rung[kRejectRungs] = {0, 0, 0, 0, 0, 0}; };

static void soundness_of(const char* what, const Model& m, int k, int dtype, uint64_t base_len, ull want_pairs, Rng& r, Tally& t) {
	const uint64_t nbins = 1ull << (2 * k);
	const uint32_t n_c = 16, draws = 64;
	while (t.pairs < want_pairs && t.launches < kMaxLaunches) {          // (a model that hardly ever gets a cut ends on the launches)
		const int order = (int)r.below(2);
		static const double spreads[5] = {0.0, 0.01, 0.03, 0.2, 1.0};
		const double spread = spreads[r.below(5)];
		const bool stale = r.below(8) == 0;
		auto a_len = [&]() { return (uint64_t)std::max(12.0, (double)base_len * (1.0 + spread * (2 * r.unit() - 1))); };
		const Slot q = draw_slot(r, k, nbins, a_len(), stale);
		Slot c[n_c];
		MscRejectRanges rg{};
		for (uint32_t i = 0; i < n_c; i++) { c[i] = draw_slot(r, k, nbins, a_len(), stale); widen(rg, c[i], i == 0); }
		const int32_t T = msc_fold_reject_cut(m, query_of(q), rg, nbins, dtype, order);
		t.launches++;
		if (T < 0) {
			t.no_cut++;
			// (pairs the cut does not cover: counted when close, to show that the models are not far from their thresholds)
			for (uint32_t i = 0; i < n_c; i++) {
				const uint64_t ex = std::min(c[i].s.sum, q.s.sum) - nbins;
				const Totals tt = totals_of(q, c[i], nbins, ex, ex, 0);
				bool close;
				weighted_sum(m, tt, order == MSC_RJ_CAND_FIRST ? c[i].s : q.s, order == MSC_RJ_CAND_FIRST ? q.s : c[i].s, nbins, dtype, &close);
				t.close_uncovered += close;
			}
			continue;
		}
		for (int i = 0; i < kRejectRungs; i++) if (msc_fold_reject_rung(i) == (uint32_t)T) t.rung[i]++;
		for (uint32_t i = 0; i < n_c; i++) {
			const uint64_t ex_c = c[i].s.sum - nbins, ex_q = q.s.sum - nbins;
			for (uint32_t d = 0; d < draws; d++) {
				const uint64_t U = r.ends((uint64_t)T), xx = std::min(c[i].x, q.x);
				const uint64_t s_max = std::min(std::min(ex_c, ex_q), U + xx + c[i].g), d_max = U + xx + c[i].g * q.e_max;
				const Totals tt = totals_of(q, c[i], nbins, r.ends(s_max), r.ends(d_max), r.ends(c[i].rk_dev + q.rk_dev));
				bool close;
				const double s = weighted_sum(m, tt, order == MSC_RJ_CAND_FIRST ? c[i].s : q.s, order == MSC_RJ_CAND_FIRST ? q.s : c[i].s, nbins, dtype, &close);
				t.pairs++;
				if (close) {
					if (t.bad++ < 5)
						fprintf(stderr, "FAILED %s: a pair under the cut T = %d is close (s = %.9g): order %d, U %llu, manh %llu, dot %llu, emd %llu, query (%llu %llu %llu %llu), candidate (%llu %llu %llu %llu)\n",
						        what, T, s, order, (ull)U, (ull)tt.manh, (ull)tt.dot, (ull)tt.emd, (ull)q.s.mag, (ull)q.s.len, (ull)q.s.sum, (ull)q.s.sq, (ull)c[i].s.mag, (ull)c[i].s.len,
						        (ull)c[i].s.sum, (ull)c[i].s.sq);
				}
			}
		}
	}
}

// the outcomes without a certificate, one by one, on a launch that otherwise gets a cut: -> the number that came out wrong
static ull edge_cases(const Model& m, int k, int dtype) {
	const uint64_t N = 1ull << (2 * k);
	const MscRejectQuery q{N + 992, 1000, N + 992, N + 3 * 992 + 10, 3000000, 30, 2};
	const MscRejectRanges c{N + 985, N + 999, 993, 1007, N + 985, N + 999, N + 2950, N + 3060, 3100000, 11};
	ull wrong = 0;
	auto expect = [&](const char* what, const Model& md, const MscRejectQuery& qq, const MscRejectRanges& cc, bool cut) {
		for (int order = 0; order < 2; order++) {
			const int32_t T = msc_fold_reject_cut(md, qq, cc, N, dtype, order);
			if ((T >= 0) != cut) { fprintf(stderr, "FAILED edge case: %s, order %d: T = %d\n", what, order, T); wrong++; }
		}
	};
	expect("the launch as it is", m, q, c, true);
	MscRejectRanges r = c; r.len_lo = 0;
	expect("a zero length among the candidates", m, q, r, false);
	MscRejectQuery z = q; z.len = 0;
	expect("a query of zero length", m, z, c, false);
	r = c; r.sum_lo = N - 1;
	expect("a sum below 4^k (a zero count)", m, q, r, false);
	r = c; r.sq_hi = 1ull << 31;
	expect("a scalar of 2^31", m, q, r, false);
	r = c; r.mag_lo = r.mag_hi + 1;
	expect("an empty range", m, q, r, false);
	r = c; r.g_hi = 1ull << 31;
	expect("a list longer than its pitch", m, q, r, false);
	Model bad = m; bad.s_min[0] = NAN;
	expect("a NaN in the model's image", bad, q, c, false);
	bad = m; bad.s_w[1] = INFINITY;
	expect("an infinite weight", bad, q, c, false);
	bad = m; bad.screen_ok = 0;
	expect("a model without an f32 image", bad, q, c, false);
	bad = m; bad.single_flag[0] = 1ull << 7;
	expect("a statistic outside the nine", bad, q, c, false);
	return wrong;
}

static int run_soundness(int argc, char** argv) {
	if (argc < 4) return 2;
	const int n_models = atoi(argv[2]);
	const ull per_model = strtoull(argv[3], nullptr, 10);
	Rng r{20260003};
	ull bad = 0, total = 0, with_cut = 0, full = 0, covered_launches = 0, close_uncovered = 0;
	for (int f = 4; f < argc; f++) {
		Model m;
		int k = 0;
		if (!parse_weights(argv[f], m, &k) || !m.screen_ok) { fprintf(stderr, "FAILED: cannot read %s\n", argv[f]); return 1; }
		const int dtype = strstr(argv[f], "u16") ? 16 : 32;
		if (f == 4) {          // (the first file: a model that cuts the launch of edge_cases)
			const ull wrong = edge_cases(m, k, dtype);
			printf("edge cases without a certificate: %llu wrong\n", wrong);
			bad += wrong;
		}
		Tally t;
		soundness_of(argv[f], m, k, dtype, 1000, per_model, r, t);
		printf("%s (k %d, %d-bit): %llu launches, %llu without a cut, rungs %llu %llu %llu %llu %llu %llu, %llu pairs under the cut, %llu of them close\n", argv[f], k, dtype, t.launches,
		       t.no_cut, t.rung[0], t.rung[1], t.rung[2], t.rung[3], t.rung[4], t.rung[5], t.pairs, t.bad);
		bad += t.bad; total += t.pairs; with_cut += t.launches > t.no_cut; full += t.pairs >= per_model; covered_launches += t.launches - t.no_cut; close_uncovered += t.close_uncovered;
	}
	for (int i = 0; i < n_models; i++) {
		const int k = r.below(2) ? 9 : 8;
		static const int dtypes[3] = {16, 32, 64};
		const int dtype = dtypes[r.below(3)];
		static const uint64_t lens[4] = {300, 1000, 1000, 3000};
		const uint64_t len = lens[r.below(4)];
		const Model m = random_model(r, k, 1ull << (2 * k), dtype, len);
		Tally t;
		char what[64];
		snprintf(what, sizeof what, "random model %d", i);
		soundness_of(what, m, k, dtype, len, per_model, r, t);
		printf("%s: statistics", what);
		for (int s = 0; s < m.n_singles; s++) printf(" 2^%d", __builtin_ctzll(m.single_flag[s]));
		printf("\n");
		printf("%s (k %d, %d-bit, %d combos, %d singles): %llu launches, %llu without a cut, rungs %llu %llu %llu %llu %llu %llu, %llu pairs, %llu close under the cut\n", what, k, dtype,
		       m.n_combos, m.n_singles, t.launches, t.no_cut, t.rung[0], t.rung[1], t.rung[2], t.rung[3], t.rung[4], t.rung[5], t.pairs, t.bad);
		bad += t.bad; total += t.pairs; with_cut += t.launches > t.no_cut; full += t.pairs >= per_model; covered_launches += t.launches - t.no_cut; close_uncovered += t.close_uncovered;
	}
	printf("soundness: %llu pairs under a cut, %llu models with a cut, %llu models with %llu pairs or more, %llu launches with a cut, %llu close pairs where there was none, %llu certified and close\n",
	       total, with_cut, full, per_model, covered_launches, close_uncovered, bad);
	if (bad == 0 && with_cut > 0) printf("fold reject soundness ok\n");
	return bad == 0 && with_cut > 0 ? 0 : 1;
}

// ---------------------------------------------------------------- a sample of sequences, as the mirrors hold it
struct Seq {
	std::vector<uint32_t> ranks;                            // the counted k-mers in bin order, a bin as often as it was counted (msc_emd_ranks.hip)
	std::vector<std::pair<uint32_t, uint32_t>> bins;        // (bin, e) for e >= 1, by bin
	std::vector<std::pair<uint32_t, uint32_t>> large;       // ... for e >= 2: the list of large bins
	std::vector<uint64_t> folded;                           // presence bits of the folded bins
	Slot slot;
};

static Seq build_seq(const std::string& s, int k, uint64_t nbins, uint32_t fold) {
	Seq o;
	const uint64_t nbf = nbins / fold;
	for (size_t i = 0; i + k <= s.size(); i++) {
		uint32_t b = 0;
		bool ok = true;
		for (int j = 0; j < k; j++) {
			const char ch = s[i + j];
			const int code = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
			if (code < 0) { ok = false; break; }
			b = b * 4 + (uint32_t)code;          // first base most significant
		}
		if (ok) o.ranks.push_back(b);
	}
	std::sort(o.ranks.begin(), o.ranks.end());
	o.folded.assign((nbf + 63) / 64, 0);
	uint64_t sq = nbins, distinct_f = 0;
	o.slot.g = 0; o.slot.e_max = 1;
	for (size_t i = 0; i < o.ranks.size();) {
		size_t j = i;
		while (j < o.ranks.size() && o.ranks[j] == o.ranks[i]) j++;
		const uint32_t e = (uint32_t)(j - i);
		o.bins.push_back({o.ranks[i], e});
		sq += (uint64_t)e * e + 2 * e;
		if (e >= 2) { o.large.push_back({o.ranks[i], e}); o.slot.g += e - 1; if (e > o.slot.e_max) o.slot.e_max = e; }
		const uint64_t fb = o.ranks[i] & (nbf - 1);          // msc_fold_bin_of
		if (!((o.folded[fb >> 6] >> (fb & 63)) & 1)) { o.folded[fb >> 6] |= 1ull << (fb & 63); distinct_f++; }
		i = j;
	}
	o.slot.s = Side{nbins + o.ranks.size(), s.size(), nbins + o.ranks.size(), sq};
	o.slot.x = (uint32_t)(o.bins.size() - distinct_f);          // k_kb_fold: distinct k-mers less distinct folded bins
	o.slot.rk_dev = 0;
	return o;
}

static int run_sample(int argc, char** argv) {
	if (argc < 9) return 2;
	std::ifstream in(argv[2]);
	Model m;
	int k_file = 0;
	if (!in || !parse_weights(argv[3], m, &k_file)) { fprintf(stderr, "FAILED: cannot read the inputs\n"); return 1; }
	const int k = atoi(argv[4]), dtype = atoi(argv[5]), order = atoi(argv[6]);
	const size_t family = (size_t)atoi(argv[7]), stride = (size_t)atoi(argv[8]);
	const uint64_t nbins = 1ull << (2 * k);
	const uint32_t fold = 16;
	std::vector<Seq> seqs;
	std::string line;
	while (std::getline(in, line)) if (!line.empty()) seqs.push_back(build_seq(line, k, nbins, fold));
	const size_t n = seqs.size();
	if (n == 0 || family == 0 || stride == 0) return 2;
	// the rank moments at the set's pitch (msc_ranks_pitch, k_rank_moments)
	size_t longest = 0;
	for (const Seq& s : seqs) longest = std::max(longest, s.ranks.size());
	const uint64_t pitch = std::max<uint64_t>(256, (longest + 255) / 256 * 256);
	MscRejectRanges rg{};
	for (size_t i = 0; i < n; i++) {
		Seq& s = seqs[i];
		uint64_t dev = 0;
		for (uint64_t t = 0; t < pitch; t++) {
			const int64_t a = t < s.ranks.size() ? (int64_t)s.ranks[t] : (int64_t)nbins, base = (int64_t)(t * nbins / pitch);
			dev += (uint64_t)(a > base ? a - base : base - a);
		}
		s.slot.rk_dev = dev;
		widen(rg, s.slot, i == 0);
	}
	printf("sample: %zu sequences, k %d, %d-bit, order %d; ranges: length %llu..%llu, sum %llu..%llu, squares %llu..%llu, moment <= %llu, G %llu\n", n, k, dtype, order, (ull)rg.len_lo,
	       (ull)rg.len_hi, (ull)rg.sum_lo, (ull)rg.sum_hi, (ull)rg.sq_lo, (ull)rg.sq_hi, (ull)rg.rk_dev_hi, (ull)rg.g_hi);
	std::vector<int32_t> cuts;
	std::vector<uint8_t> rejected;
	ull rung[kRejectRungs + 1] = {0, 0, 0, 0, 0, 0, 0}, unrelated = 0, unrelated_under = 0, related = 0, related_under = 0, bad = 0;
	double worst = -1e300;
	for (size_t qi = 0; qi < n; qi += stride) {
		const Seq& q = seqs[qi];
		const int32_t T = msc_fold_reject_cut(m, query_of(q.slot), rg, nbins, dtype, order);
		cuts.push_back(T);
		int at = kRejectRungs;
		for (int i = 0; i < kRejectRungs; i++) if (T >= 0 && msc_fold_reject_rung(i) == (uint32_t)T) at = i;
		rung[at]++;
		for (size_t ci = 0; ci < n; ci++) {
			const Seq& c = seqs[ci];
			// the folded product: P1' over the presence bits, P2' = the query's large bins by FOLDED bin (e - 1 each) the candidate's folded row holds
			uint64_t U = 0;
			for (size_t w = 0; w < q.folded.size(); w++) U += (uint64_t)__builtin_popcountll(q.folded[w] & c.folded[w]);
			for (const auto& en : q.large) {
				const uint64_t fb = en.first & (nbins / fold - 1);
				if ((c.folded[fb >> 6] >> (fb & 63)) & 1) U += en.second - 1;
			}
			const bool rel = qi / family == ci / family, under = T >= 0 && U <= (uint64_t)T;
			rejected.push_back(under);
			(rel ? related : unrelated)++;
			if (under) (rel ? related_under : unrelated_under)++;
			if (!under) continue;
			// the pair's true reductions: the two lists of counted bins merged, the ranks walked at the pitch
			uint64_t S = 0, D = 0, emd = 0;
			for (size_t a = 0, b = 0; a < q.bins.size() && b < c.bins.size();) {
				if (q.bins[a].first < c.bins[b].first) a++;
				else if (q.bins[a].first > c.bins[b].first) b++;
				else { S += std::min(q.bins[a].second, c.bins[b].second); D += (uint64_t)q.bins[a].second * c.bins[b].second; a++; b++; }
			}
			for (uint64_t t = 0; t < pitch; t++) {
				const int64_t a = t < q.ranks.size() ? (int64_t)q.ranks[t] : (int64_t)nbins, b = t < c.ranks.size() ? (int64_t)c.ranks[t] : (int64_t)nbins;
				emd += (uint64_t)(a > b ? a - b : b - a);
			}
			const Totals tt = totals_of(q.slot, c.slot, nbins, S, D, emd);
			bool close;
			const double s = weighted_sum(m, tt, order == MSC_RJ_CAND_FIRST ? c.slot.s : q.slot.s, order == MSC_RJ_CAND_FIRST ? q.slot.s : c.slot.s, nbins, dtype, &close);
			if (s > worst) worst = s;
			if (close && bad++ < 5) fprintf(stderr, "FAILED: pair (%zu, %zu) is under the cut %d with U = %llu and close, s = %.9g\n", qi, ci, T, (ull)U, s);
		}
	}
	printf("cuts over %zu queries: T=0 %llu, 32 %llu, 64 %llu, 128 %llu, 256 %llu, 512 %llu, none %llu\n", cuts.size(), rung[0], rung[1], rung[2], rung[3], rung[4], rung[5], rung[6]);
	printf("unrelated pairs under their query's cut: %llu of %llu; related: %llu of %llu; the largest FP64 sum of a rejected pair %.6g; rejected and close: %llu\n", unrelated_under, unrelated,
	       related_under, related, worst, bad);
	printf("gate %.6f\n", unrelated ? (double)unrelated_under / (double)unrelated : 0.0);
	if (argc > 9) {
		FILE* f = fopen(argv[9], "wb");
		if (!f) return 1;
		const bool ok = fwrite(cuts.data(), sizeof(int32_t), cuts.size(), f) == cuts.size() && fwrite(rejected.data(), 1, rejected.size(), f) == rejected.size();
		fclose(f);
		if (!ok) return 1;
	}
	if (bad == 0) printf("fold reject sample ok\n");
	return bad == 0 ? 0 : 1;
}

int main(int argc, char** argv) {
	if (argc >= 2 && !strcmp(argv[1], "soundness")) return run_soundness(argc, argv);
	if (argc >= 2 && !strcmp(argv[1], "sample")) return run_sample(argc, argv);
	fprintf(stderr, "usage: fold_reject_check soundness <models> <pairs per model> <weights file> ... | sample <sequences> <weights file> <k> <dtype> <order> <family> <query stride> [<out>]\n");
	return 2;
}
