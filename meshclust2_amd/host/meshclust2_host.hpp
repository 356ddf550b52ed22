// meshclust2_host.hpp -- C++ host-side mirror of the reference's classes for the hot path, over the C ABI.
//
// The reference reaches the path through template member calls:
//   Loader<T>::get_point            clutil/Loader.cpp:112-179
//   Feature<T>::compute / operator() predict/Feature.h:197-239
//   Trainer<T>::get_close / filter / merge / closest   cluster/Trainer.cpp:23-157
//   Predictor<T>::close / similarity predict/Predictor.cpp:255-333
// This header gives a maintainer the same names and argument meaning with device-resident points: a Point is a
// (set, slot) handle instead of a heap DivergencePoint<T>*, errors are C++ exceptions again (msc::Error carries the
// msc_status the ABI returned), and T is the reference's run-time datatype (8/16/32/64) instead of a template
// parameter. Header-only; link against libmeshclust2_hip.so.
#pragma once
#include <cstdint>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/meshclust2_hip.h"

namespace msc {

struct Error : std::runtime_error {
	int code;
	Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

class Context {
public:
	explicit Context(int device = 0) {
		int rc = msc_create(device, &h_);
		if (rc != MSC_OK) throw Error(rc, msc_last_error(nullptr));
	}
	~Context() { msc_destroy(h_); }
	Context(const Context&) = delete;
	Context& operator=(const Context&) = delete;
	msc_ctx* get() const { return h_; }
	void set_kernel_timing(bool on) { check(msc_set_kernel_timing(h_, on ? 1 : 0)); }
	// search_pairs with a divergence-statistic model on the matrix-core route (sums from cells; agrees with the default to rounding, not bit for bit)
	void set_pairs_div_cells(bool on) { check(msc_set_pairs_div_cells(h_, on ? 1 : 0)); }
	// score_multi with a divergence statistic on the matrix-core route, no merge pass per query (integer statistics bit-equal, the two sums to 1e-9)
	void set_multi_div_cells(bool on) { check(msc_set_multi_div_cells(h_, on ? 1 : 0)); }
	void set_emd_bounds(bool on) { check(msc_set_emd_bounds(h_, on ? 1 : 0)); }
	// ... and their product over presence bits folded fold-to-1 (0: off; 8, 16 or 32), exact counts for the pairs the screen leaves open (identical flags)
	void set_fold_screen(int fold) { check(msc_set_fold_screen(h_, fold)); }
	// the queries' side of up to cap consecutive full blocks of a Q x M call in one set of launches (0, 1: block by block; identical results)
	void set_query_groups(int cap) { check(msc_set_query_groups(h_, cap)); }
	void set_tail_groups(int cap) { check(msc_set_tail_groups(h_, cap)); }
	// a folded block's rows get an integer cut: pairs whose folded product output lies under it are "not close" without an evaluation (identical flags)
	void set_fold_reject(bool on) { check(msc_set_fold_reject(h_, on ? 1 : 0)); }
	// Q x M calls over two sparse sets on the matrix-core route, mirrors built from their lists (identical results)
	void set_sparse_matrix_pass(bool on) { check(msc_set_sparse_matrix_pass(h_, on ? 1 : 0)); }
	void check(int rc) const { if (rc != MSC_OK) throw Error(rc, msc_last_error(h_)); }
private:
	msc_ctx* h_ = nullptr;
};

// The `points` vector of the reference (cluster/CRunner.cpp:505-544), resident in HBM.
class PointSet {
public:
	// sparse_entries > 0: sparse layout (sorted (bin, value) lists) able to hold that many stored bins in total
	PointSet(Context& ctx, int k, int datatype_bits, uint64_t capacity, uint64_t sparse_entries = 0) : ctx_(ctx) {
		if (sparse_entries) ctx_.check(msc_hist_set_create_sparse(ctx_.get(), k, datatype_bits, capacity, sparse_entries, &h_));
		else ctx_.check(msc_hist_set_create(ctx_.get(), k, datatype_bits, capacity, &h_));
	}
	~PointSet() { msc_hist_set_destroy(h_); }
	PointSet(const PointSet&) = delete;
	PointSet& operator=(const PointSet&) = delete;
	msc_hist_set* get() const { return h_; }
	Context& ctx() const { return ctx_; }
	uint64_t capacity() const { return msc_hist_set_capacity(h_); }
	void clear() { ctx_.check(msc_hist_set_clear(ctx_.get(), h_)); }      // sparse sets: every slot empty, the whole arena free

	// Loader<T>::get_point for a batch. strip = the std::string overload (drops non-ACGT first).
	void get_points(uint64_t first_slot, const std::vector<std::string>& seqs, bool strip = false) { get_points(first_slot, seqs.data(), seqs.size(), strip); }
	// ... n sequences of a longer list, where they lie (no copies)
	void get_points(uint64_t first_slot, const std::string* seqs, size_t n, bool strip = false) {
		std::vector<const char*> p(n);
		std::vector<uint64_t> l(n);
		for (size_t i = 0; i < n; i++) { p[i] = seqs[i].data(); l[i] = seqs[i].size(); }
		ctx_.check(msc_hist_build(ctx_.get(), h_, first_slot, n, p.data(), l.data(), strip ? 1 : 0));
	}
	msc_hist_info info(uint64_t slot) const {
		msc_hist_info i;
		ctx_.check(msc_hist_info_get(ctx_.get(), h_, slot, &i));
		return i;
	}
	uint64_t get_length(uint64_t slot) const { return info(slot).length; }
	std::vector<uint64_t> get_lengths(uint64_t first, uint64_t n) const {
		std::vector<uint64_t> out(n);
		ctx_.check(msc_hist_lengths(ctx_.get(), h_, first, n, out.data()));
		return out;
	}
	template <class T> std::vector<T> get_data(uint64_t slot) const {     // DivergencePoint::points, natural order
		std::vector<T> v((size_t)1 << (2 * msc_hist_set_k(h_)));
		ctx_.check(msc_hist_download(ctx_.get(), h_, slot, v.data()));
		return v;
	}
	// Center(c) takes c->clone(); centre->set(*next) keeps the stale magnitude (clutil/DivergencePoint.cpp:182-190)
	void clone(uint64_t dst, const PointSet& src, uint64_t src_slot) { ctx_.check(msc_hist_clone(ctx_.get(), h_, dst, src.h_, src_slot)); }
	void set(uint64_t dst, const PointSet& src, uint64_t src_slot) { ctx_.check(msc_hist_assign(ctx_.get(), h_, dst, src.h_, src_slot)); }
	void copy(uint64_t dst, const PointSet& src, uint64_t src_slot) { ctx_.check(msc_hist_copy(ctx_.get(), h_, dst, src.h_, src_slot)); }
	void clone_batch(const std::vector<uint32_t>& dst, const PointSet& src, const std::vector<uint32_t>& src_slots) {
		ctx_.check(msc_hist_clone_batch(ctx_.get(), h_, dst.data(), src.h_, src_slots.data(), dst.size()));
	}
	void copy_batch(const std::vector<uint32_t>& dst, const PointSet& src, const std::vector<uint32_t>& src_slots) {
		ctx_.check(msc_hist_copy_batch(ctx_.get(), h_, dst.data(), src.h_, src_slots.data(), dst.size()));
	}
	// slot dst[i] of this set = the reverse complement of slot src_slots[i] of src (msc_hist_revcomp_batch: bins'[b] = bins[rc(b)], the record
	// copied with its 1-mers reversed); no in-place form
	void revcomp_batch(const std::vector<uint32_t>& dst, const PointSet& src, const std::vector<uint32_t>& src_slots) {
		if (dst.size() != src_slots.size()) throw Error(MSC_ERR_INVALID_ARG, "revcomp_batch: one source slot per destination slot");
		ctx_.check(msc_hist_revcomp_batch(ctx_.get(), h_, dst.data(), src.h_, src_slots.data(), dst.size()));
	}
	// slot dst[i] of this set = the strand-neutral form of slot src_slots[i] of src (msc_hist_canonical_batch: bins'[b] = bins[b] + bins[rc(b)] - 1,
	// clamped; a sequence and its reverse complement give the same slot); src may be this set and src_slots[i] == dst[i]: in place
	void canonical_batch(const std::vector<uint32_t>& dst, const PointSet& src, const std::vector<uint32_t>& src_slots) {
		if (dst.size() != src_slots.size()) throw Error(MSC_ERR_INVALID_ARG, "canonical_batch: one source slot per destination slot");
		ctx_.check(msc_hist_canonical_batch(ctx_.get(), h_, dst.data(), src.h_, src_slots.data(), dst.size()));
	}
private:
	Context& ctx_;
	msc_hist_set* h_ = nullptr;
};

// Feature<T> (finalised) + the GLM weights of one block of a weights file.
class Feature {
public:
	Feature(Context& ctx, const std::string& weights_file, int block = 0) : ctx_(ctx) {
		ctx_.check(msc_model_load(ctx_.get(), weights_file.c_str(), block, &h_));
	}
	~Feature() { msc_model_destroy(h_); }
	Feature(const Feature&) = delete;
	Feature& operator=(const Feature&) = delete;
	msc_model* get() const { return h_; }
	size_t size() const { return (size_t)msc_model_n_combos(h_); }          // Feature::size()
	int n_singles() const { return msc_model_n_singles(h_); }

	// cache = feat->compute(*a_i, *b) for every candidate a_i: rows of normalised singles (the `cache` vectors)
	std::vector<double> compute(const PointSet& cands, const std::vector<uint32_t>& slots, const PointSet& q, uint64_t q_slot,
	                            int order = MSC_ORDER_CAND_FIRST, std::vector<double>* combos = nullptr,
	                            std::vector<double>* sums = nullptr) const {
		std::vector<double> singles(slots.size() * (size_t)n_singles());
		if (combos) combos->resize(slots.size() * size());
		if (sums) sums->resize(slots.size());
		ctx_.check(msc_score(ctx_.get(), h_, cands.get(), slots.data(), slots.size(), q.get(), q_slot, order, singles.data(),
		                     combos ? combos->data() : nullptr, sums ? sums->data() : nullptr, nullptr));
		return singles;
	}
	// the same for an explicit list of pairs (a_slots[i] of a, b_slots[i] of b) in one call (msc_score_pair_list; the reference's table walks
	// a vector<pair<Point*, Point*>>, predict/FeatureSelector.cpp:23-33): rows of normalised singles in the caller's order
	std::vector<double> compute_pairs(const PointSet& a, const std::vector<uint32_t>& a_slots, const PointSet& b, const std::vector<uint32_t>& b_slots,
	                                  int order = MSC_ORDER_CAND_FIRST, std::vector<double>* combos = nullptr, std::vector<double>* sums = nullptr) const {
		if (a_slots.size() != b_slots.size()) throw Error(MSC_ERR_INVALID_ARG, "compute_pairs: the two slot lists are one pair list");
		std::vector<double> singles(a_slots.size() * (size_t)n_singles());
		if (combos) combos->resize(a_slots.size() * size());
		if (sums) sums->resize(a_slots.size());
		ctx_.check(msc_score_pair_list(ctx_.get(), h_, a.get(), a_slots.data(), b.get(), b_slots.data(), a_slots.size(), order, 0, nullptr, singles.data(),
		                               combos ? combos->data() : nullptr, sums ? sums->data() : nullptr, nullptr, nullptr));
		return singles;
	}
private:
	Context& ctx_;
	msc_model* h_ = nullptr;
};

// cluster/Trainer.{h,cpp}, scoring half. `cutoff` is Trainer::cutoff as given on the command line (--id).
class Trainer {
public:
	Trainer(Context& ctx, const std::string& weights_file, double cutoff) : ctx_(ctx), feat_(ctx, weights_file, 0), cutoff_(cutoff) {}
	double get_id() const { return cutoff_ > 1 ? cutoff_ / 100.0 : cutoff_; }

	// std::tuple<Point<T>*,double,size_t,size_t> get_close(Point<T>*, bvec_iterator istart, iend, bool& is_min)
	// -> (position in `window` of the arg-max or -1, similarity, close flags); the caller owns the bvec bookkeeping.
	std::tuple<int64_t, double, std::vector<uint8_t>> get_close(const PointSet& points, const std::vector<uint32_t>& window,
	                                                            const PointSet& q, uint64_t q_slot, bool& is_min) const {
		std::vector<uint8_t> flags(window.size());
		int64_t pos = -1;
		double sim = -1;
		int im = 1;
		ctx_.check(msc_get_close(ctx_.get(), feat_.get(), cutoff_, points.get(), window.data(), window.size(), q.get(), q_slot,
		                         flags.data(), &pos, &sim, &im));
		is_min = im != 0;
		return std::make_tuple(pos, sim, std::move(flags));
	}
	// void filter(Point<T>*, vector<pair<Point<T>*,bool>>&): erases the rejected entries
	void filter(const PointSet& centre_set, uint64_t centre, const PointSet& points, std::vector<uint32_t>& vec) const {
		std::vector<uint8_t> keep(vec.size());
		uint64_t n = 0;
		ctx_.check(msc_filter(ctx_.get(), feat_.get(), cutoff_, centre_set.get(), centre, points.get(), vec.data(), vec.size(), keep.data(), &n));
		size_t w = 0;
		for (size_t i = 0; i < vec.size(); i++) if (keep[i]) vec[w++] = vec[i];
		vec.resize(w);
	}
	// long merge(vector<Center<T>>& centers, long current, long begin, long last)
	long merge(const PointSet& centres, const std::vector<uint32_t>& centre_slots, long current, long begin, long last) const {
		int64_t best = 0;
		ctx_.check(msc_merge(ctx_.get(), feat_.get(), cutoff_, centres.get(), centre_slots.data(), centre_slots.size(), current, begin, last, &best));
		return (long)best;
	}
	// Point<T>* closest(Point<double>* mean, vector<...>&) fused with the mean that precedes it (get_mean / mean_shift_update)
	int64_t closest(const PointSet& points, const std::vector<uint32_t>& members) const {
		int64_t pos = -1;
		ctx_.check(msc_mean_nearest(ctx_.get(), points.get(), members.data(), members.size(), &pos, nullptr, nullptr));
		return pos;
	}
	const Feature& feature() const { return feat_; }
private:
	Context& ctx_;
	Feature feat_;
	double cutoff_;
};

// Predictor<T>::close + similarity for one query against a database chunk (fastcar/FC_Runner.cpp:426-471). Like work(), it
// follows the file's mode (predict/Predictor.h:20-21): a `mode: 1` file (classification only: what meshclust2 --dump and
// msc_train_class write) gives similarity 1 for every close pair, a `mode: 2` file (regression only) calls every pair close.
class Predictor {
public:
	Predictor(Context& ctx, const std::string& weights_file) : ctx_(ctx) {
		std::ifstream in(weights_file.c_str());
		std::string tok;
		unsigned mode = 0;
		while (in >> tok) if (tok == "mode:") { in >> mode; break; }
		if (!(mode & 3)) throw Error(MSC_ERR_IO, "weights file " + weights_file + ": no `mode:` line with a classification or regression block");
		if (mode & 1) cls_.reset(new Feature(ctx, weights_file, 0));
		if (mode & 2) reg_.reset(new Feature(ctx, weights_file, 1));
	}
	uint8_t get_mode() const { return (uint8_t)((cls_ ? 1 : 0) | (reg_ ? 2 : 0)); }
	void search(const PointSet& db, const std::vector<uint32_t>& slots, const PointSet& q, uint64_t q_slot, std::vector<uint8_t>& close,
	            std::vector<double>& similarity) const {
		close.resize(slots.size());
		similarity.resize(slots.size());
		ctx_.check(msc_search(ctx_.get(), cls_ ? cls_->get() : nullptr, reg_ ? reg_->get() : nullptr, db.get(), slots.data(), slots.size(), q.get(), q_slot,
		                      close.data(), similarity.data()));
	}
	// search() for an explicit list of pairs (a_slots[i] of db against query b_slots[i] of q): msc_search's rules per pair, one
	// msc_score_pair_list call per block of the weights file
	void score_pairs(const PointSet& db, const std::vector<uint32_t>& a_slots, const PointSet& q, const std::vector<uint32_t>& b_slots, std::vector<uint8_t>& close,
	                 std::vector<double>& similarity) const {
		if (a_slots.size() != b_slots.size()) throw Error(MSC_ERR_INVALID_ARG, "score_pairs: the two slot lists are one pair list");
		const size_t n = a_slots.size();
		close.assign(n, 1);
		similarity.assign(n, 1.0);
		if (n == 0) return;
		if (cls_)
			ctx_.check(msc_score_pair_list(ctx_.get(), cls_->get(), db.get(), a_slots.data(), q.get(), b_slots.data(), n, MSC_ORDER_CAND_FIRST, 0, nullptr, nullptr, nullptr,
			                               nullptr, nullptr, close.data()));
		if (reg_) {
			ctx_.check(msc_score_pair_list(ctx_.get(), reg_->get(), db.get(), a_slots.data(), q.get(), b_slots.data(), n, MSC_ORDER_CAND_FIRST, 0, nullptr, nullptr, nullptr,
			                               similarity.data(), nullptr, nullptr));
			for (double& v : similarity) v = v < 0 ? 0 : (v > 1 ? 1 : v);      // p_predict clamps to [0,1], predict/Predictor.cpp:293-298
		}
	}
	// the same for a block of queries in ONE pass over the database window (msc_score_multi: each candidate tile fetched from HBM
	// serves 16 queries): close[q * slots.size() + i], similarity likewise. Values are bit-identical to search() per query.
	void search_block(const PointSet& db, const std::vector<uint32_t>& slots, const PointSet& q, const std::vector<uint32_t>& q_slots,
	                  std::vector<uint8_t>& close, std::vector<double>& similarity) const {
		const size_t n = slots.size() * q_slots.size();
		close.assign(n, 1);
		similarity.assign(n, 1.0);
		if (n == 0) return;
		if (cls_)
			ctx_.check(msc_score_multi(ctx_.get(), cls_->get(), db.get(), slots.data(), slots.size(), q.get(), q_slots.data(), q_slots.size(), MSC_ORDER_CAND_FIRST,
			                           nullptr, nullptr, close.data(), 0, nullptr));
		if (reg_) {
			ctx_.check(msc_score_multi(ctx_.get(), reg_->get(), db.get(), slots.data(), slots.size(), q.get(), q_slots.data(), q_slots.size(), MSC_ORDER_CAND_FIRST,
			                           similarity.data(), nullptr, nullptr, 0, nullptr));
			for (double& v : similarity) v = v < 0 ? 0 : (v > 1 ? 1 : v);      // p_predict clamps to [0,1], predict/Predictor.cpp:293-298
		}
	}
	// the same block with only the close pairs as output (msc_search_pairs): pair (q, i) is listed when win_lo[q] <= i < win_hi[q] and close;
	// query q's pairs are [offsets[q], offsets[q + 1]) of cand_idx (index into slots, ascending) and similarity -- the values of search()
	std::vector<uint64_t> search_pairs(const PointSet& db, const std::vector<uint32_t>& slots, const PointSet& q, const std::vector<uint32_t>& q_slots,
	                                   const std::vector<uint64_t>& win_lo, const std::vector<uint64_t>& win_hi, std::vector<uint32_t>& cand_idx,
	                                   std::vector<double>& similarity, msc_pairs_info* info = nullptr) const {
		if (win_lo.size() != q_slots.size() || win_hi.size() != q_slots.size()) throw Error(MSC_ERR_INVALID_ARG, "search_pairs: one window per query");
		std::vector<uint64_t> offsets(q_slots.size() + 1, 0);
		msc_pairs_info inf;
		ctx_.check(msc_search_pairs(ctx_.get(), cls_ ? cls_->get() : nullptr, reg_ ? reg_->get() : nullptr, db.get(), slots.data(), slots.size(), q.get(), q_slots.data(),
		                            q_slots.size(), win_lo.data(), win_hi.data(), offsets.data(), &inf));
		cand_idx.resize(inf.n_pairs);
		similarity.resize(inf.n_pairs);
		ctx_.check(msc_search_pairs_fetch(ctx_.get(), 0, inf.n_pairs, cand_idx.data(), similarity.data()));
		if (info) *info = inf;
		return offsets;
	}
	// search_pairs with each query's list cut on the device to its top_n pairs of largest similarity (msc_search_pairs_top: ties to the lower
	// index, the kept pairs in ascending index with the bits search_pairs gives; top_n = 0 is no cut). close_counts (nullable) = pairs per
	// query before the cut. Empty windows mean every candidate.
	std::vector<uint64_t> search_pairs_top(const PointSet& db, const std::vector<uint32_t>& slots, const PointSet& q, const std::vector<uint32_t>& q_slots,
	                                       const std::vector<uint64_t>& win_lo, const std::vector<uint64_t>& win_hi, uint32_t top_n, std::vector<uint32_t>& cand_idx,
	                                       std::vector<double>& similarity, std::vector<uint64_t>* close_counts = nullptr, msc_pairs_info* info = nullptr) const {
		const bool windows = !win_lo.empty() || !win_hi.empty();
		if (windows && (win_lo.size() != q_slots.size() || win_hi.size() != q_slots.size())) throw Error(MSC_ERR_INVALID_ARG, "search_pairs_top: one window per query");
		std::vector<uint64_t> offsets(q_slots.size() + 1, 0);
		if (close_counts) close_counts->assign(q_slots.size(), 0);
		msc_pairs_info inf;
		ctx_.check(msc_search_pairs_top(ctx_.get(), cls_ ? cls_->get() : nullptr, reg_ ? reg_->get() : nullptr, db.get(), slots.data(), slots.size(), q.get(), q_slots.data(),
		                                q_slots.size(), windows ? win_lo.data() : nullptr, windows ? win_hi.data() : nullptr, top_n, offsets.data(),
		                                close_counts ? close_counts->data() : nullptr, &inf));
		cand_idx.resize(inf.n_pairs);
		similarity.resize(inf.n_pairs);
		ctx_.check(msc_search_pairs_fetch(ctx_.get(), 0, inf.n_pairs, cand_idx.data(), similarity.data()));
		if (info) *info = inf;
		return offsets;
	}
	// search_pairs on both strands (msc_search_pairs_strands): per query the union of its list and of its reverse complement's, ascending index;
	// strand[p] = 0 (the query as given; also a tie) or 1 (its reverse complement gave the larger similarity, or the only one). Empty windows
	// mean every candidate.
	std::vector<uint64_t> search_pairs_strands(const PointSet& db, const std::vector<uint32_t>& slots, const PointSet& q, const std::vector<uint32_t>& q_slots,
	                                           const std::vector<uint64_t>& win_lo, const std::vector<uint64_t>& win_hi, std::vector<uint32_t>& cand_idx,
	                                           std::vector<double>& similarity, std::vector<uint8_t>& strand, msc_pairs_info* info = nullptr) const {
		const bool windows = !win_lo.empty() || !win_hi.empty();
		if (windows && (win_lo.size() != q_slots.size() || win_hi.size() != q_slots.size())) throw Error(MSC_ERR_INVALID_ARG, "search_pairs_strands: one window per query");
		std::vector<uint64_t> offsets(q_slots.size() + 1, 0);
		msc_pairs_info inf;
		ctx_.check(msc_search_pairs_strands(ctx_.get(), cls_ ? cls_->get() : nullptr, reg_ ? reg_->get() : nullptr, db.get(), slots.data(), slots.size(), q.get(), q_slots.data(),
		                                    q_slots.size(), windows ? win_lo.data() : nullptr, windows ? win_hi.data() : nullptr, offsets.data(), &inf));
		cand_idx.resize(inf.n_pairs);
		similarity.resize(inf.n_pairs);
		strand.resize(inf.n_pairs);
		ctx_.check(msc_search_pairs_fetch(ctx_.get(), 0, inf.n_pairs, cand_idx.data(), similarity.data()));
		ctx_.check(msc_search_pairs_fetch_strands(ctx_.get(), 0, inf.n_pairs, strand.data()));
		if (info) *info = inf;
		return offsets;
	}
private:
	Context& ctx_;
	std::unique_ptr<Feature> cls_, reg_;
};

// The global-alignment identity of listed pairs (msc_align_pairs: the reference's GlobAlignE, what Feature::align computes with the default
// parameters, predict/Feature.cpp:697-718): pair p aligns seqs[first[p]] -- the definition's sequence 1, ties are not symmetric -- with
// seqs[second[p]]; sequences of 1 .. 32 767 bytes, compared byte by byte. identity[p] = matches[p] / length[p]; the caller's order.
struct Alignments {
	std::vector<int32_t> score, length, matches;
	std::vector<double> identity;
};
namespace detail {
inline Alignments align_full(const Context& ctx, bool long_entry, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second, int match,
                             int mismatch, int gap_open, int gap_continue) {
	if (first.size() != second.size()) throw Error(MSC_ERR_INVALID_ARG, "align_pairs: first and second are one pair list");
	std::string text;
	std::vector<uint64_t> offsets(1, 0);
	for (const std::string& s : seqs) { text += s; offsets.push_back(text.size()); }
	text.push_back('\0');          // (never a null pointer, whatever the list holds)
	Alignments a;
	const size_t n = first.size();
	a.score.resize(n); a.length.resize(n); a.matches.resize(n); a.identity.resize(n);
	const uint8_t* bytes = reinterpret_cast<const uint8_t*>(text.data());
	if (long_entry)
		ctx.check(msc_align_pairs_long(ctx.get(), bytes, offsets.data(), seqs.size(), first.data(), second.data(), n, match, mismatch, gap_open, gap_continue, a.score.data(), a.length.data(),
		                               a.matches.data()));
	else
		ctx.check(msc_align_pairs(ctx.get(), bytes, offsets.data(), seqs.size(), first.data(), second.data(), n, match, mismatch, gap_open, gap_continue, a.score.data(), a.length.data(),
		                          a.matches.data()));
	for (size_t i = 0; i < n; i++) a.identity[i] = (double)a.matches[i] / a.length[i];
	return a;
}
}  // namespace detail
inline Alignments align_pairs(const Context& ctx, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second, int match = 1,
                              int mismatch = -1, int gap_open = 2, int gap_continue = 1) {
	return detail::align_full(ctx, false, seqs, first, second, match, mismatch, gap_open, gap_continue);
}
// align_pairs for sequences of 1 .. 1 048 575 bytes (msc_align_pairs_long): the same integers; pairs within align_pairs's limit
// run on its kernels
inline Alignments align_pairs_long(const Context& ctx, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second, int match = 1,
                                   int mismatch = -1, int gap_open = 2, int gap_continue = 1) {
	return detail::align_full(ctx, true, seqs, first, second, match, mismatch, gap_open, gap_continue);
}

// align_pairs's integers and the alignment itself (msc_align_pairs_trace): pair p's runs are ops[op_offsets[p]] ..
// ops[op_offsets[p + 1]), the columns in forward order, one word per run = run << 4 | op with BAM's op numbers -- 7 '=', 8 'X', 1 'I' (consumes
// seqs[first[p]], the query), 2 'D' (consumes seqs[second[p]], the reference). Sequences of 1 .. 32 767 bytes.
struct Traces : Alignments {
	std::vector<uint64_t> op_offsets;
	std::vector<uint32_t> ops;
	std::string cigar(size_t p) const {          // such as "120=1X3I"
		std::string s;
		for (uint64_t k = op_offsets.at(p); k < op_offsets.at(p + 1); k++) { s += std::to_string(ops[k] >> 4); s += "MIDNSHP=X*******"[ops[k] & 15u]; }
		return s;
	}
};
inline Traces align_pairs_trace(const Context& ctx, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second, int match = 1,
                                int mismatch = -1, int gap_open = 2, int gap_continue = 1) {
	if (first.size() != second.size()) throw Error(MSC_ERR_INVALID_ARG, "align_pairs_trace: first and second are one pair list");
	std::string text;
	std::vector<uint64_t> offsets(1, 0);
	for (const std::string& s : seqs) { text += s; offsets.push_back(text.size()); }
	text.push_back('\0');          // (never a null pointer, whatever the list holds)
	Traces a;
	const size_t n = first.size();
	a.score.resize(n); a.length.resize(n); a.matches.resize(n); a.identity.resize(n);
	a.op_offsets.assign(n + 1, 0);
	ctx.check(msc_align_pairs_trace(ctx.get(), reinterpret_cast<const uint8_t*>(text.data()), offsets.data(), seqs.size(), first.data(), second.data(), n, match, mismatch, gap_open,
	                                gap_continue, a.score.data(), a.length.data(), a.matches.data(), a.op_offsets.data()));
	a.ops.resize(a.op_offsets[n]);
	ctx.check(msc_align_pairs_trace_fetch(ctx.get(), 0, a.ops.size(), a.ops.data()));
	for (size_t i = 0; i < n; i++) a.identity[i] = (double)a.matches[i] / a.length[i];
	return a;
}

// The same integers over a band of diagonals (msc_align_pairs_banded, msc_align_pairs_auto). align_pairs_banded fills the
// diagonals within `band` of the corner-to-corner ones and says per pair whether its integers are PROVEN to be align_pairs's (certified[p]
// = 1); align_pairs_auto doubles each pair's band from first_band (0: the library's default) until it is, and always returns align_pairs's
// integers -- band_used[p] is the band that certified the pair, no_band where the full grid was filled.
struct BandedAlignments {
	enum : uint32_t { no_band = 0xffffffffu };
	std::vector<int32_t> score, length, matches;
	std::vector<double> identity;
	std::vector<uint8_t> certified;          // align_pairs_banded
	std::vector<uint32_t> band_used;         // align_pairs_auto
};
namespace detail {
inline BandedAlignments align_over_a_band(const Context& ctx, bool automatic, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second,
                                          uint32_t band, int match, int mismatch, int gap_open, int gap_continue, bool long_entry = false) {
	if (first.size() != second.size()) throw Error(MSC_ERR_INVALID_ARG, "align_pairs: first and second are one pair list");
	std::string text;
	std::vector<uint64_t> offsets(1, 0);
	for (const std::string& s : seqs) { text += s; offsets.push_back(text.size()); }
	text.push_back('\0');
	BandedAlignments a;
	const size_t n = first.size();
	a.score.resize(n); a.length.resize(n); a.matches.resize(n); a.identity.resize(n);
	const uint8_t* bytes = reinterpret_cast<const uint8_t*>(text.data());
	if (automatic) {
		a.band_used.resize(n + 1);          // (never a null pointer: NULL means "not wanted")
		if (long_entry)
			ctx.check(msc_align_pairs_long_auto(ctx.get(), bytes, offsets.data(), seqs.size(), first.data(), second.data(), n, match, mismatch, gap_open, gap_continue, band, a.score.data(),
			                                    a.length.data(), a.matches.data(), a.band_used.data()));
		else
			ctx.check(msc_align_pairs_auto(ctx.get(), bytes, offsets.data(), seqs.size(), first.data(), second.data(), n, match, mismatch, gap_open, gap_continue, band, a.score.data(),
			                               a.length.data(), a.matches.data(), a.band_used.data()));
		a.band_used.resize(n);
	} else {
		a.certified.resize(n);
		if (long_entry)
			ctx.check(msc_align_pairs_long_banded(ctx.get(), bytes, offsets.data(), seqs.size(), first.data(), second.data(), n, match, mismatch, gap_open, gap_continue, band, a.score.data(),
			                                      a.length.data(), a.matches.data(), a.certified.data()));
		else
			ctx.check(msc_align_pairs_banded(ctx.get(), bytes, offsets.data(), seqs.size(), first.data(), second.data(), n, match, mismatch, gap_open, gap_continue, band, a.score.data(),
			                                 a.length.data(), a.matches.data(), a.certified.data()));
	}
	for (size_t i = 0; i < n; i++) a.identity[i] = (double)a.matches[i] / a.length[i];
	return a;
}
}  // namespace detail
inline BandedAlignments align_pairs_banded(const Context& ctx, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second, uint32_t band,
                                           int match = 1, int mismatch = -1, int gap_open = 2, int gap_continue = 1) {
	return detail::align_over_a_band(ctx, false, seqs, first, second, band, match, mismatch, gap_open, gap_continue);
}
inline BandedAlignments align_pairs_auto(const Context& ctx, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second,
                                         uint32_t first_band = 0, int match = 1, int mismatch = -1, int gap_open = 2, int gap_continue = 1) {
	return detail::align_over_a_band(ctx, true, seqs, first, second, first_band, match, mismatch, gap_open, gap_continue);
}
// both for sequences of 1 .. 1 048 575 bytes (msc_align_pairs_long_banded, msc_align_pairs_long_auto)
inline BandedAlignments align_pairs_long_banded(const Context& ctx, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second,
                                                uint32_t band, int match = 1, int mismatch = -1, int gap_open = 2, int gap_continue = 1) {
	return detail::align_over_a_band(ctx, false, seqs, first, second, band, match, mismatch, gap_open, gap_continue, true);
}
inline BandedAlignments align_pairs_long_auto(const Context& ctx, const std::vector<std::string>& seqs, const std::vector<uint32_t>& first, const std::vector<uint32_t>& second,
                                              uint32_t first_band = 0, int match = 1, int mismatch = -1, int gap_open = 2, int gap_continue = 1) {
	return detail::align_over_a_band(ctx, true, seqs, first, second, first_band, match, mismatch, gap_open, gap_continue, true);
}

// the other strand of a sequence as a string: reversed, A <-> T and C <-> G, every other byte as it is
inline std::string reverse_complement(const std::string& s) {
	std::string rc(s.rbegin(), s.rend());
	for (char& c : rc) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
	return rc;
}

}  // namespace msc
