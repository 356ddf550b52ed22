// msc_fold_reject.h -- the integer cut of a folded block (msc_fold.h): for one query and the RANGES of a launch's
// candidates, whether "not close" is proven for every candidate whose folded product output is small. Shared by the kernels and host code;
// free of HIP, so that tests/fold_reject_check.cpp builds it with g++ alone.
//
// A folded product gives P1' and P2' with 0 <= P1 <= P1' + min(x_q, x_c), 0 <= P2 <= P2' (pair_features.hip, k_pair_epilogue_bits_bound).
// Let U = P1' + P2' and take an integer T. For every pair with U <= T, with e = count - 1 the excess counts (msc_pair_gemm.hip):
//     S = sum min(e_q, e_c) = P1 + sum over the bins large in both of (min(e_q, e_c) - 1)      in [0, T + x_q + G]
//     D = sum e_q e_c       = P1 + P2 + sum over the candidate's large bins of (e_c - 1) e_q   in [0, T + x_q + G e_max_q]
// G = the largest sum of (e_c - 1) over a candidate's list of large bins, e_max_q = the query's largest excess count (at least 1). Also
// S <= min(ex_c, ex_q) with ex = sum - 4^k, and the sum of products sum c_i q_i <= (sq_c + sq_q) / 2 -- the caps k_pair_epilogue_bits_bound
// applies. The two reductions every statistic reads are then
//     manh = ex_c + ex_q - 2 S          dot = 4^k + ex_c + ex_q + D
// The candidate's scalars (mag, length, sum, sum of squares) lie in the ranges of the launch, each taken on its own; the query's are known;
// the earth mover's distance lies in [0, max rk_dev_c + rk_dev_q] (msc_emd_list.hip). Over that box every raw statistic gets an interval from
// the monotonicity arguments written beside it below; the intervals pass through the normalisation, the combo products and the weighted sum
// of screen_close (pair_features.hip) as intervals, and the cut certifies when the upper end of s lies below 0.
//
// The arithmetic is FP64 on integers below 2^32, widened OUTWARD by kRejectEps = 2^-20 -- screen_close's kScreenEps -- of the operands'
// magnitudes at every operation: far more than FP64 rounds, and enough for the one thing that is f32 here, the model's image (s_min, s_inv,
// s_w are the FP64 constants rounded to f32, 2^-24 each; the difference r - s_min is widened by both magnitudes, so a cancelling
// subtraction is covered too). The FP64 evaluation that decides a flag (epilogue_eval) rounds at 2^-53 per operation.
//
// There is NO certificate -- never a guess -- when
//   * a statistic is not one of the nine below, or the model has no f32 image;
//   * similarity_ratio on 32-bit bins unless the whole box wraps exactly once or not at all (screen_raw_box's rule);
//   * a length of zero lies in range (length_difference throws), a sum below 4^k (a zero count), an empty range;
//   * a value of 2^31 or more among the scalars (manhattan is read through `int`; sq_a sq_b must fit 64 bits), a pearson denominator
//     that is not positive over the whole box;
//   * anything comes out NaN or infinite (every comparison with a NaN is false, and the last one is `upper end < -margin`).
#pragma once
#include <math.h>
#include <stdint.h>

#include "msc_layout.h"

// the statistics, by their bits in meshclust2_hip.h (MSC_FEAT_*); the header stands without it
#define MSC_RJ_MANHATTAN          (1ULL << 2)
#define MSC_RJ_EUCLIDEAN          (1ULL << 3)
#define MSC_RJ_NORMALIZED_VECTORS (1ULL << 5)
#define MSC_RJ_PEARSON_COEFF      (1ULL << 9)
#define MSC_RJ_INTERSECTION       (1ULL << 13)
#define MSC_RJ_EMD                (1ULL << 18)
#define MSC_RJ_LENGTHD            (1ULL << 21)
#define MSC_RJ_KULCZYNSKI2        (1ULL << 27)
#define MSC_RJ_SIMRATIO           (1ULL << 28)

// combo kinds and argument orders as in meshclust2_hip.h (MSC_COMBO_*, MSC_ORDER_*)
enum { MSC_RJ_XY = 0, MSC_RJ_XY2 = 1, MSC_RJ_X2Y = 2, MSC_RJ_X2Y2 = 3 };
enum { MSC_RJ_CAND_FIRST = 0, MSC_RJ_QUERY_FIRST = 1 };

constexpr double kRejectEps = 9.5367431640625e-07;      // 2^-20 = kScreenEps
constexpr double kRejectMargin = 1e-9;                   // s < -margin: 1 / (1 + exp(-s)) rounds below 0.5 in FP64, the flag is 0
constexpr int32_t kRejectNoCut = -1;
constexpr int kRejectRungs = 6;

// the ladder: T(q) is the largest rung that certifies
MSC_HD uint32_t msc_fold_reject_rung(int i) { return i == 0 ? 0u : 16u << i; }      // 0, 32, 64, 128, 256, 512

// One query: its scalar record's four, the second rank moment (k_rank_moments), its own collisions (k_kb_fold) and its largest excess
// count (the largest e of its list of large bins; 1 without a list).
struct MscRejectQuery {
	uint64_t mag, len, sum, sq, rk_dev;
	uint32_t x, e_max;
};

// The candidates of a launch -- or of the whole set, which is wider and as sound: minima and maxima of the same quantities per slot, and
// g_hi = the largest sum of (e - 1) over a slot's list of large bins.
struct MscRejectRanges {
	uint64_t mag_lo, mag_hi, len_lo, len_hi, sum_lo, sum_hi, sq_lo, sq_hi, rk_dev_hi, g_hi;
};

struct MscRejectIv { double lo, hi; };

// ---- intervals, every result widened outward
MSC_HD MscRejectIv msc_rj_out(double lo, double hi, double mag) {
	const double w = kRejectEps * mag + 1e-300;
	return MscRejectIv{lo - w, hi + w};
}
MSC_HD MscRejectIv msc_rj_iv(double lo, double hi) { return msc_rj_out(lo, hi, fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi)); }
MSC_HD double msc_rj_abs(const MscRejectIv& a) { return fabs(a.lo) > fabs(a.hi) ? fabs(a.lo) : fabs(a.hi); }
MSC_HD MscRejectIv msc_rj_scale(const MscRejectIv& a, double k) { return k >= 0 ? msc_rj_iv(a.lo * k, a.hi * k) : msc_rj_iv(a.hi * k, a.lo * k); }
MSC_HD MscRejectIv msc_rj_mul(const MscRejectIv& a, const MscRejectIv& b) {
	const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
	double lo = p0, hi = p0;
	if (p1 < lo) lo = p1;
	if (p2 < lo) lo = p2;
	if (p3 < lo) lo = p3;
	if (p1 > hi) hi = p1;
	if (p2 > hi) hi = p2;
	if (p3 > hi) hi = p3;
	if (!(lo <= hi)) return MscRejectIv{NAN, NAN};      // (a NaN among the products)
	return msc_rj_iv(lo, hi);
}
MSC_HD MscRejectIv msc_rj_sq(const MscRejectIv& a) {
	if (a.lo >= 0) return msc_rj_iv(a.lo * a.lo, a.hi * a.hi);
	if (a.hi <= 0) return msc_rj_iv(a.hi * a.hi, a.lo * a.lo);
	const double m = msc_rj_abs(a);
	return msc_rj_iv(0.0, m * m);
}

// ---- the box of one (query, ranges, T): the two reductions and what the statistics read beside them, as numbers below 2^34
struct MscRejectBox {
	double N, T;
	double mag_q, len_q, sum_q, sq_q, ex_q;
	double mag_lo, mag_hi, len_lo, len_hi, sum_lo, sum_hi, sq_lo, sq_hi, ex_lo, ex_hi;      // the candidate's
	double s_hi, d_hi;                  // S in [0, s_hi], D in [0, d_hi]
	double manh_lo, manh_hi;            // manh = ex_c + ex_q - 2 S
	double dot_lo, dot_hi;              // dot = N + ex_c + ex_q + D, cut to (sq_c + sq_q) / 2
	double e_lo, e_hi;                  // E = sq_c + sq_q - 2 dot >= 0: the squared euclidean distance
	double emd_hi;
	bool cand_first;
	int dtype;
};

MSC_HD bool msc_fold_reject_box(const MscRejectQuery& q, const MscRejectRanges& c, uint64_t nbins, int dtype, int order, uint32_t T, MscRejectBox& b) {
	const uint64_t lim = 1ull << 31;
	if (c.mag_lo > c.mag_hi || c.len_lo > c.len_hi || c.sum_lo > c.sum_hi || c.sq_lo > c.sq_hi) return false;
	if (q.len == 0 || c.len_lo == 0 || q.mag == 0 || c.mag_lo == 0) return false;
	if (q.sum < nbins || c.sum_lo < nbins || nbins == 0 || nbins >= lim) return false;
	if (q.mag >= lim || q.len >= lim || q.sum >= lim || q.sq >= lim || c.mag_hi >= lim || c.len_hi >= lim || c.sum_hi >= lim || c.sq_hi >= lim) return false;
	if (q.rk_dev >= (1ull << 52) || c.rk_dev_hi >= (1ull << 52) || c.g_hi >= lim || q.e_max >= (1u << 20) || T >= (1u << 20)) return false;
	b.N = (double)nbins; b.T = (double)T; b.dtype = dtype; b.cand_first = order == MSC_RJ_CAND_FIRST;
	b.mag_q = (double)q.mag; b.len_q = (double)q.len; b.sum_q = (double)q.sum; b.sq_q = (double)q.sq; b.ex_q = (double)(q.sum - nbins);
	b.mag_lo = (double)c.mag_lo; b.mag_hi = (double)c.mag_hi; b.len_lo = (double)c.len_lo; b.len_hi = (double)c.len_hi;
	b.sum_lo = (double)c.sum_lo; b.sum_hi = (double)c.sum_hi; b.sq_lo = (double)c.sq_lo; b.sq_hi = (double)c.sq_hi;
	b.ex_lo = (double)(c.sum_lo - nbins); b.ex_hi = (double)(c.sum_hi - nbins);
	const double e_max = q.e_max < 1 ? 1.0 : (double)q.e_max, G = (double)c.g_hi;
	// (every value here is an integer below 2^53: the sums and differences are exact)
	double s_hi = b.T + (double)q.x + G;
	if (s_hi > b.ex_q) s_hi = b.ex_q;
	if (s_hi > b.ex_hi) s_hi = b.ex_hi;
	b.s_hi = s_hi;
	b.d_hi = b.T + (double)q.x + G * e_max;
	// manh is increasing in ex_c and decreasing in S: its ends are at (ex_hi, 0) and (ex_lo, s_hi); and it is a sum of absolute values
	b.manh_hi = b.ex_hi + b.ex_q;
	b.manh_lo = b.ex_lo + b.ex_q - 2.0 * s_hi;
	if (b.manh_lo < 0) b.manh_lo = 0;
	// dot is increasing in ex_c and in D; the cap by the squares is increasing in sq_c
	b.dot_lo = b.N + b.ex_lo + b.ex_q;
	const double dot_open = b.N + b.ex_hi + b.ex_q + b.d_hi, dot_top = 0.5 * (b.sq_hi + b.sq_q);
	b.dot_hi = dot_open < dot_top ? dot_open : dot_top;
	if (b.dot_hi < b.dot_lo) return false;          // (never for true histograms)
	// E is increasing in sq_c and decreasing in dot; it is a sum of squares
	b.e_hi = b.sq_hi + b.sq_q - 2.0 * b.dot_lo;
	b.e_lo = b.sq_lo + b.sq_q - 2.0 * dot_open;
	if (b.e_lo < 0) b.e_lo = 0;
	if (b.e_hi < b.e_lo) return false;
	b.emd_hi = (double)c.rk_dev_hi + (double)q.rk_dev;
	return b.manh_hi < (double)lim;
}

// The interval of one raw statistic over the box; false: no enclosure. a / b below = first / second argument of the reference call; every
// statistic but similarity_ratio on 32-bit bins is symmetric in the two.
MSC_HD bool msc_fold_reject_raw(uint64_t flag, const MscRejectBox& b, MscRejectIv& r) {
	switch (flag) {
	case MSC_RJ_MANHATTAN:
		// = manh (read through `int`: msc_fold_reject_box keeps it below 2^31): increasing in manh
		r = msc_rj_iv(b.manh_lo, b.manh_hi);
		return true;
	case MSC_RJ_EUCLIDEAN:
		// = sqrt(E): increasing in E >= 0
		r = msc_rj_iv(sqrt(b.e_lo), sqrt(b.e_hi));
		return true;
	case MSC_RJ_NORMALIZED_VECTORS:
		// = dot / sqrt(sq_a sq_b), dot > 0: increasing in dot, decreasing in sq_c
		r = msc_rj_iv(b.dot_lo / sqrt(b.sq_hi * b.sq_q), b.dot_hi / sqrt(b.sq_lo * b.sq_q));
		return true;
	case MSC_RJ_PEARSON_COEFF: {
		// = dt / sqrt(np nq) with (predict/Feature.cpp:800-810, the means from the STORED mag; d = mag - sum, 0 for a histogram as built)
		//     np = sq_a - 2 (mag_a / N) sum_a + mag_a^2 / N = sq_a - sum_a^2 / N + d_a^2 / N      (likewise nq)
		//     dt = dot - (mag_b sum_a + mag_a sum_b - mag_a mag_b) / N = dot - (sum_a sum_b - d_a d_b) / N
		//        = D - ex_a ex_b / N + d_a d_b / N                    (dot = N + ex_a + ex_b + D, sum = N + ex)
		// np: increasing in sq_c, decreasing in sum_c (> 0), increasing in d_c^2. dt: increasing in D, decreasing in ex_c (ex_q >= 0),
		// linear in d_c at the query's fixed d_q. The quotient: increasing in dt; in np nq decreasing where dt >= 0, increasing where dt < 0.
		const double dq = b.mag_q - b.sum_q, dc_lo = b.mag_lo - b.sum_hi, dc_hi = b.mag_hi - b.sum_lo;
		const MscRejectIv dc2 = msc_rj_sq(MscRejectIv{dc_lo, dc_hi});
		const double nq = b.sq_q - b.sum_q * b.sum_q / b.N + dq * dq / b.N;
		const double np_lo = b.sq_lo - b.sum_hi * b.sum_hi / b.N + dc2.lo / b.N, np_hi = b.sq_hi - b.sum_lo * b.sum_lo / b.N + dc2.hi / b.N;
		const MscRejectIv nn = msc_rj_mul(msc_rj_out(np_lo, np_hi, b.sq_hi + b.sum_hi * b.sum_hi / b.N), msc_rj_out(nq, nq, b.sq_q + b.sum_q * b.sum_q / b.N));
		if (!(nn.lo > 0)) return false;
		const double x0 = dc_lo * dq, x1 = dc_hi * dq;
		const double dt_lo = 0.0 - b.ex_hi * b.ex_q / b.N + (x0 < x1 ? x0 : x1) / b.N, dt_hi = b.d_hi - b.ex_lo * b.ex_q / b.N + (x0 > x1 ? x0 : x1) / b.N;
		const MscRejectIv dt = msc_rj_out(dt_lo, dt_hi, b.d_hi + b.ex_hi * b.ex_q / b.N + (fabs(x0) > fabs(x1) ? fabs(x0) : fabs(x1)) / b.N);
		const double s_lo = sqrt(nn.lo), s_hi = sqrt(nn.hi);
		r = msc_rj_iv(dt.lo / (dt.lo >= 0 ? s_hi : s_lo), dt.hi / (dt.hi >= 0 ? s_lo : s_hi));
		return true;
	}
	case MSC_RJ_INTERSECTION:
		// = 2 floor((sum_a + sum_b - manh) / 2) / (mag_a + mag_b), and sum_a + sum_b - manh = 2 N + 2 S exactly: = 2 (N + S) / (mag_a + mag_b),
		// increasing in S (non-increasing in manh), decreasing in mag_c
		r = msc_rj_iv(2.0 * b.N / (b.mag_hi + b.mag_q), 2.0 * (b.N + b.s_hi) / (b.mag_lo + b.mag_q));
		return true;
	case MSC_RJ_EMD:
		// the distance itself, in [0, rk_dev_c + rk_dev_q]
		r = msc_rj_iv(0.0, b.emd_hi);
		return true;
	case MSC_RJ_LENGTHD: {
		// = | len_a - len_b | (both > 0): convex in len_c, 0 where the query's length lies in range, largest at an end
		const double d0 = fabs(b.len_q - b.len_lo), d1 = fabs(b.len_q - b.len_hi);
		const bool inside = b.len_q >= b.len_lo && b.len_q <= b.len_hi;
		r = msc_rj_iv(inside ? 0.0 : (d0 < d1 ? d0 : d1), d0 > d1 ? d0 : d1);
		return true;
	}
	case MSC_RJ_KULCZYNSKI2: {
		// = coeff (N + S), coeff = N (ap + aq) / (2 ap aq) with ap = mag_a / N: = (N^2 / 2) (1 / mag_a + 1 / mag_b) > 0, decreasing in mag_c;
		// the product is increasing in S (non-increasing in manh)
		const double h = 0.5 * b.N * b.N;
		r = msc_rj_iv(h * (1.0 / b.mag_hi + 1.0 / b.mag_q) * b.N, h * (1.0 / b.mag_lo + 1.0 / b.mag_q) * (b.N + b.s_hi));
		return true;
	}
	case MSC_RJ_SIMRATIO: {
		// = dot / (dot + sqrt(W)), dot > 0, W >= 0: increasing in dot at fixed W, decreasing in W at fixed dot -- bounded over the box of the
		// two, as screen_raw_box does. W = E for bins that are not 32 bits wide. For 32-bit bins W = (E - 2^33 neg) mod 2^64 with
		// neg = (manh - (sum_a - sum_b)) / 2 = ex_b - S, the second argument's excess that the first does not match: neg = 0 over the whole
		// box: W = E; 1 <= neg < 2^30 over the whole box (E < 2^33 by the limits of msc_fold_reject_box): W = 2^64 + E - 2^33 neg at every
		// point, increasing in E, decreasing in neg. Anything else straddles a wrap: no enclosure.
		double w_lo = b.e_lo, w_hi = b.e_hi;
		if (b.dtype == 32) {
			const double exb_lo = b.cand_first ? b.ex_q : b.ex_lo, exb_hi = b.cand_first ? b.ex_q : b.ex_hi;
			const double neg_lo = exb_lo - b.s_hi, neg_hi = exb_hi;      // (neg = ex_b - S is increasing in ex_b, decreasing in S)
			if (neg_hi != 0) {
				if (neg_lo < 1 || neg_hi >= 1073741824.0 || b.e_hi >= 8589934592.0) return false;
				const double two64 = 18446744073709551616.0, two33 = 8589934592.0;
				w_lo = two64 + b.e_lo - two33 * neg_hi;
				w_hi = two64 + b.e_hi - two33 * neg_lo;
				// (2^64 + E - 2^33 neg rounds to FP64 at 2^-53 of 2^64: the widening below covers it)
			}
		}
		const MscRejectIv w = msc_rj_iv(w_lo < 0 ? 0 : w_lo, w_hi);
		r = msc_rj_iv(b.dot_lo / (b.dot_lo + sqrt(w.hi)), b.dot_hi / (b.dot_hi + sqrt(w.lo < 0 ? 0 : w.lo)));
		return true;
	}
	default:
		return false;
	}
}

// Whether s < 0 is proven for every candidate in the ranges whose product output satisfies P1' + P2' <= T. Model: any struct with the
// fields of MscDevModel's f32 image (msc_internal.h) -- n_singles, n_combos, single_flag, is_sim, combo_kind, combo_n, combo_idx, s_min,
// s_inv, s_w, screen_ok. The normalisation, the products and the sum are screen_close's, on intervals.
template <class Model>
MSC_HD bool msc_fold_reject_certifies(const Model& md, const MscRejectQuery& q, const MscRejectRanges& c, uint64_t nbins, int dtype, int order, uint32_t T) {
	if (!md.screen_ok) return false;
	MscRejectBox box;
	if (!msc_fold_reject_box(q, c, nbins, dtype, order, T, box)) return false;
	auto single = [&](int i, MscRejectIv& v) -> bool {
		MscRejectIv r;
		if (!msc_fold_reject_raw(md.single_flag[i], box, r)) return false;
		const double mn = (double)md.s_min[i], inv = (double)md.s_inv[i];
		const MscRejectIv d = msc_rj_out(r.lo - mn, r.hi - mn, msc_rj_abs(r) + fabs(mn));
		const MscRejectIv u = msc_rj_scale(d, inv);
		v = md.is_sim[i] ? u : msc_rj_out(1.0 - u.hi, 1.0 - u.lo, 1.0 + msc_rj_abs(u));
		return msc_rj_abs(v) < 1e150;      // (false for a NaN or an infinity at either end)
	};
	double s = (double)md.s_w[0];
	s += kRejectEps * fabs(s);
	for (int col = 0; col < md.n_combos; col++) {
		const int kind = md.combo_kind[col];
		const bool two = md.combo_n[col] == 2 || kind == MSC_RJ_XY2 || kind == MSC_RJ_X2Y;
		MscRejectIv x, y{1.0, 1.0};
		if (!single(md.combo_idx[col][0], x)) return false;
		if (two && !single(md.combo_idx[col][1], y)) return false;
		MscRejectIv d;
		switch (kind) {
		case MSC_RJ_XY:   d = msc_rj_mul(x, y); break;
		case MSC_RJ_X2Y2: d = msc_rj_mul(msc_rj_sq(x), msc_rj_sq(y)); break;
		case MSC_RJ_XY2:  d = msc_rj_mul(x, msc_rj_sq(y)); break;
		default:          d = msc_rj_mul(msc_rj_sq(x), y); break;
		}
		const MscRejectIv t = msc_rj_scale(d, (double)md.s_w[col + 1]);
		s += t.hi + kRejectEps * (fabs(s) + fabs(t.hi));      // the upper end of the sum so far
	}
	return s < -kRejectMargin;      // (false for a NaN)
}

// T(q): the largest rung of the ladder that certifies, or kRejectNoCut. The box grows with T, so the rungs are tried from the top.
template <class Model>
MSC_HD int32_t msc_fold_reject_cut(const Model& md, const MscRejectQuery& q, const MscRejectRanges& c, uint64_t nbins, int dtype, int order) {
	for (int i = kRejectRungs - 1; i >= 0; i--)
		if (msc_fold_reject_certifies(md, q, c, nbins, dtype, order, msc_fold_reject_rung(i))) return (int32_t)msc_fold_reject_rung(i);
	return kRejectNoCut;
}
