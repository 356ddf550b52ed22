// msc_fastcar.cpp -- query x database identity search over the GPU hot path.
//
// The second caller of the path in the reference: fastcar (fastcar/FC_Runner.cpp). For every query, the database
// sequences inside its length window that the classification model calls "close" are reported with the regression
// model's identity estimate:  <query> \t <db> \t <100 * similarity>.  The loop structure, the per-chunk unstable
// std::sort by length, bin_search, format_header and the output formatting follow fastcar/FC_Runner.cpp:389-471,
// 560-611 at one thread (one output file "<prefix>0"); training is out of scope, a two-block weights file is required.
//
//   msc_fastcar <db.fa> --query <q.fa> --recover weights.txt [--output output] [--chunk 10000] [--no-format] [--device 0] [--div-cells] [--top N] [--both-strands] [--canonical] [--align] [--align-band W] [--cigar]
//
// --align: one more column after the predicted identity (and after the strand column where there is one): the identity of the global alignment of
// the reported pair, matches / length of msc_align_pairs_long with the default parameters (1, -1, 2, 1), the query as the first sequence -- the quantity
// the column before it predicts -- printed the same way, 100 * identity. The hits of one (query chunk, database chunk) step are aligned in one
// call, over the strings as read from the files (1 .. 1 048 575 bytes each; pairs within 32 767 bytes run on msc_align_pairs's kernels); with --both-strands a `-` hit aligns the query's reverse complement
// (the string reversed, A <-> T, C <-> G, any other byte kept). Not together with --canonical: a strand-neutral point has no orientation to
// align. Without the flag the output is what it was.
// --align-band W (with --align): the same column through msc_align_pairs_long_auto, which fills a band of diagonals per pair (first half-width W, 0 = the
// library's default, doubled until the pair is certified) and returns msc_align_pairs_long's integers: the output is byte for byte that of --align.
// --cigar (with --align, not beside --align-band): one more last column, the alignment itself as a CIGAR string such as 120=1X3I (msc_align_pairs_trace,
// = equal bytes, X different bytes, I consumes the query, D consumes the database entry; the query is the CIGAR's query, reversed
// for a `-` hit as --align aligns it). A hit with a sequence longer than 32 767 bytes prints * there; its identity column still comes from
// msc_align_pairs_long. Without --cigar every output byte is what it was.
//
// --canonical: database and query histograms are made strand-neutral right after they are built (msc_hist_canonical_batch, in place: each k-mer
// counted together with its reverse complement), so a query and its reverse complement give the same lines; everything else is unchanged. The
// model should have been trained on such histograms (msc_cluster --canonical). Not together with --both-strands: that flag compares the
// query's two strands with the entry as stored and reports which one hit, a different definition of "both strands".
//
// --both-strands: every block of queries, single-member blocks included, goes through msc_search_pairs_strands: a hit is reported when the query
// or its reverse complement is close to the database entry as stored, with the larger of the two similarities (a tie goes to the query as
// given) and a last column + or -. Not together with --top.
//
// --top N: each query's N best hits over the whole database (the rule of msc_search_pairs_top: largest similarity, ties to the earlier
// database chunk and then to the lower position in the chunk's window order). Per database chunk the cut runs on the device; across
// chunks at most N survivors per chunk and query are merged here by the same rule, and a query's lines are written once every database
// chunk of its query chunk is done, in the order they would have had without the flag.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <memory>
#include <string>
#include <vector>

#include "meshclust2_host.hpp"

namespace {

struct Rec { std::string header, seq; };

bool safe_getline(std::istream& is, std::string& t) {
	t.clear();
	std::streambuf* sb = is.rdbuf();
	for (;;) {
		int c = sb->sbumpc();
		if (c == '\n') return true;
		if (c == '\r') { if (sb->sgetc() == '\n') sb->sbumpc(); return true; }
		if (c == std::streambuf::traits_type::eof()) { if (t.empty()) { is.setstate(std::ios::eofbit); return false; } return true; }
		t += (char)c;
	}
}

// SingleFileLoader::next (clutil/SingleFileLoader.cpp:45-83): continuation lines that start with blank extend the header
std::vector<Rec> read_fasta(const std::string& path) {
	std::ifstream in(path.c_str());
	if (!in) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(1); }
	std::vector<Rec> out;
	std::string line;
	while (in.good()) {
		if (!safe_getline(in, line)) break;
		if (line.empty()) continue;
		if (line[0] == '>') out.push_back({line, ""});
		else if (out.empty()) continue;
		else if (line[0] == ' ' || line[0] == '\t') {
			bool all = true;
			for (char c : line) if (c != ' ' && c != '\t') all = false;
			if (!all) out.back().header += line;
		} else out.back().seq += line;
	}
	return out;
}

struct Pt { std::string header; uint64_t length; uint32_t slot; };

long bin_search(const std::vector<Pt*>& points, size_t begin, size_t last, size_t length) {      // FC_Runner.cpp:389-407
	if (last < begin) return 0;
	size_t idx = begin + (last - begin) / 2;
	if (points.at(idx)->length == length) {
		while (idx > 0 && points[idx - 1]->length == length) idx--;
		return (long)idx;
	} else if (points.at(idx)->length > length) {
		if (begin == idx) return (long)idx;
		return bin_search(points, begin, idx - 1, length);
	}
	return bin_search(points, idx + 1, last, length);
}

std::string format_header(const std::string& hdr) {                                              // FC_Runner.cpp:409-424
	long len = (long)hdr.length(), b = 0;
	if (!hdr.empty() && hdr[0] == '>') b++;
	for (long i = b; i < len; i++) if (hdr[(size_t)i] == ' ' || hdr[(size_t)i] == '\t') { len = i + 1; break; }
	return hdr.substr((size_t)b, (size_t)(len - b));
}

void load_chunk(msc::PointSet& set, const std::vector<Rec>& recs, size_t off, size_t n, std::vector<Pt>& pts, bool canonical) {
	std::vector<std::string> seqs;
	for (size_t i = 0; i < n; i++) seqs.push_back(recs[off + i].seq);
	set.get_points(0, seqs, /*strip=*/true);               // Loader<T>::get_point(header, base, ...): the string overload
	if (canonical && n) {                                  // --canonical: the strand-neutral histograms, in place (lengths do not change)
		std::vector<uint32_t> all(n);
		for (size_t i = 0; i < n; i++) all[i] = (uint32_t)i;
		set.canonical_batch(all, set, all);
	}
	pts.resize(n);
	for (size_t i = 0; i < n; i++) pts[i] = Pt{recs[off + i].header, set.get_length(i), (uint32_t)i};
}

// a hit that survived its database chunk's cut; `chunk` and `cand` give its place in the output without --top
struct Surv { size_t chunk, cand; double sim; std::string header; double aln; std::string cigar; };

// the rule of msc_search_pairs_top on the host: the n of largest similarity (compared as doubles), ties to the earlier entry, order kept
template <class T>
void cut_top(std::vector<T>& v, size_t n) {
	if (n == 0 || v.size() <= n) return;
	std::vector<size_t> order(v.size());
	for (size_t i = 0; i < order.size(); i++) order[i] = i;
	std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return v[a].sim > v[b].sim; });
	order.resize(n);
	std::sort(order.begin(), order.end());
	std::vector<T> kept;
	for (size_t i : order) kept.push_back(std::move(v[i]));
	v.swap(kept);
}

}  // namespace

int main(int argc, char** argv) {
	std::vector<std::string> files, qfiles;
	std::string weights, output = "output";
	size_t chunk = 10000, qblock = 16, top = 0;
	bool format = true, sparse = false, report_kernels = false, div_cells = false, sparse_matrix = false, both_strands = false, canonical = false, align = false, align_band = false, cigar = false;
	uint32_t first_band = 0;
	int device = 0;
	for (int i = 1; i < argc; i++) {
		std::string a = argv[i];
		auto need = [&](const char* w) { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", w); std::exit(1); } return std::string(argv[++i]); };
		if (a == "--query" || a == "-q") qfiles.push_back(need("--query"));
		else if (a == "--recover" || a == "-r") weights = need("--recover");
		else if (a == "--output" || a == "-o") output = need("--output");
		else if (a == "--chunk" || a == "-c") chunk = (size_t)std::atol(need("--chunk").c_str());
		else if (a == "--query-block") qblock = std::max<size_t>(1, (size_t)std::atol(need("--query-block").c_str()));
		else if (a == "--no-format" || a == "--noformat") format = false;
		else if (a == "--threads" || a == "-t") need("--threads");
		else if (a == "--kernels") report_kernels = true;   // after the run: the streaming kernels the library picked for the scoring passes, on stderr
		else if (a == "--sparse") sparse = true;        // sparse histogram layout (required for k >= 13; also the faster one for --feat slow models)
		else if (a == "--div-cells") div_cells = true;  // msc_set_pairs_div_cells: a --feat slow model's query blocks on the matrix-core route
		else if (a == "--sparse-matrix") sparse_matrix = true;  // msc_set_sparse_matrix_pass: with --sparse, the query blocks on the matrix-core route
		else if (a == "--top") top = (size_t)std::max(0l, std::atol(need("--top").c_str()));          // each query's N best hits (0: all)
		else if (a == "--both-strands") both_strands = true;          // msc_search_pairs_strands: the queries and their reverse complements
		else if (a == "--canonical") canonical = true;          // msc_hist_canonical_batch on every chunk: strand-neutral histograms
		else if (a == "--align") align = true;          // msc_align_pairs_long on every reported pair: a column with the alignment identity
		else if (a == "--align-band") { align_band = true; first_band = (uint32_t)std::max(0l, std::atol(need("--align-band").c_str())); }          // --align through msc_align_pairs_long_auto
		else if (a == "--cigar") cigar = true;          // with --align: msc_align_pairs_trace, a last column with the hit's CIGAR string
		else if (a == "--device") device = std::atoi(need("--device").c_str());
		else files.push_back(a);
	}
	if (files.empty() || qfiles.empty() || weights.empty()) {
		std::fprintf(stderr, "usage: %s <db.fa> --query <q.fa> --recover weights.txt [--output prefix] [--chunk 10000] [--no-format] [--sparse] [--sparse-matrix] [--div-cells] [--top N] [--both-strands] [--canonical] [--align] [--align-band W] [--cigar]\n", argv[0]);
		return 1;
	}
	if (canonical && both_strands) {
		std::fprintf(stderr, "--canonical and --both-strands cannot be combined: they are different definitions of a search on both strands\n");
		return 1;
	}
	if (canonical && align) {
		std::fprintf(stderr, "--align and --canonical cannot be combined: a strand-neutral point has no orientation to align\n");
		return 1;
	}
	if (align_band && !align) {
		std::fprintf(stderr, "--align-band needs --align: it chooses how the alignment column is computed\n");
		return 1;
	}
	if (cigar && (!align || align_band)) {
		std::fprintf(stderr, "--cigar needs --align and cannot be combined with --align-band: the CIGAR is the full-grid alignment's\n");
		return 1;
	}
	if (both_strands && top) {
		std::fprintf(stderr, "--both-strands and --top cannot be combined: the cut is not defined over two strands\n");
		return 1;
	}
	try {
		int k = 0, dtype = 16;
		double similarity = 0.9;
		{
			std::ifstream in(weights.c_str());
			std::string tok;
			while (in >> tok) {
				if (tok == "k:") in >> k;
				else if (tok == "ID:") in >> similarity;
				else if (tok == "Datatype:") { in >> tok; dtype = tok == "uint8_t" ? 8 : tok == "uint16_t" ? 16 : tok == "uint32_t" ? 32 : 64; }
				else if (tok == "n_combos:") break;
			}
		}
		msc::Context ctx(device);
		ctx.set_pairs_div_cells(div_cells);
		ctx.set_sparse_matrix_pass(sparse_matrix);
		msc::Predictor pred(ctx, weights);
		std::vector<Rec> db, queries;
		for (const auto& f : files) { auto r = read_fasta(f); db.insert(db.end(), r.begin(), r.end()); }
		for (const auto& f : qfiles) { auto r = read_fasta(f); queries.insert(queries.end(), r.begin(), r.end()); }
		// dense sets are refilled chunk after chunk; a sparse set's entry arena is append-only, so each chunk gets a fresh one
		auto bases_of = [](const std::vector<Rec>& recs, size_t off, size_t n) { uint64_t t = 0; for (size_t i = 0; i < n; i++) t += recs[off + i].seq.size(); return t; };
		auto make_set = [&](const std::vector<Rec>& recs, size_t off, size_t n) {
			return std::unique_ptr<msc::PointSet>(new msc::PointSet(ctx, k, dtype, std::max<size_t>(1, n), sparse ? (canonical ? 3 : 1) * bases_of(recs, off, n) + 1024 : 0));          // (--canonical appends a list of up to twice the entries)
		};
		std::unique_ptr<msc::PointSet> qset_p = make_set(queries, 0, std::min(chunk, queries.size()));
		std::unique_ptr<msc::PointSet> dset_p = make_set(db, 0, std::min(chunk, db.size()));
		const std::string delim = format ? "\t" : "!";
		std::ofstream out((output + "0").c_str());
		uint64_t num_pred_pos = 0;
		std::vector<std::string> kernels;
		auto note_kernel = [&] {
			char name[160];
			int q_per_read = 0;
			if (!report_kernels || msc_last_kernel_info(ctx.get(), name, sizeof name, &q_per_read) != MSC_OK) return;
			if (std::find(kernels.begin(), kernels.end(), name) == kernels.end()) kernels.push_back(name);
		};
		for (size_t qo = 0; qo < queries.size(); qo += chunk) {
			std::vector<Pt> qp;
			if (sparse && qo) qset_p = make_set(queries, qo, std::min(chunk, queries.size() - qo));
			msc::PointSet& qset = *qset_p;
			load_chunk(qset, queries, qo, std::min(chunk, queries.size() - qo), qp, canonical);
			std::vector<std::vector<Surv> > best(top ? qp.size() : 0);          // --top: each query's survivors over the database chunks so far
			size_t n_dchunks = 0;
			for (size_t d0 = 0; d0 < db.size(); d0 += chunk) {
				std::vector<Pt> dp;
				if (sparse && (d0 || qo)) dset_p = make_set(db, d0, std::min(chunk, db.size() - d0));
				msc::PointSet& dset = *dset_p;
				load_chunk(dset, db, d0, std::min(chunk, db.size() - d0), dp, canonical);
				std::vector<Pt*> pts;
				for (auto& p : dp) pts.push_back(&p);
				std::sort(pts.begin(), pts.end(), [](Pt* a, Pt* b) { return a->length < b->length; });      // FC_Runner.cpp:590-592
				if (pts.empty()) continue;
				const size_t dchunk = n_dchunks++;
				// work() (:426-471) for every query of the chunk. Queries are taken in blocks of `qblock` neighbours in LENGTH order, so
				// their length windows nearly coincide and one Q x M pass over the union window serves the block; each query then
				// keeps only its own window, and the lines are written in the reference's order (query order, then window order).
				struct Hit { size_t cand; double sim; uint8_t strand; double aln; std::string cigar; };
				std::vector<std::vector<Hit> > hits(qp.size());
				std::vector<size_t> win_start(qp.size()), win_end(qp.size());
				for (size_t qi = 0; qi < qp.size(); qi++) {
					const size_t q_len = qp[qi].length;
					const size_t begin_length = (size_t)(q_len * similarity);
					const size_t end_length = (size_t)(q_len / similarity);
					size_t s0 = (size_t)bin_search(pts, 0, pts.size() - 1, begin_length), e0 = s0;
					while (e0 < pts.size() && pts[e0]->length <= end_length) e0++;
					win_start[qi] = s0;
					win_end[qi] = e0;
				}
				std::vector<size_t> by_len(qp.size());
				for (size_t i = 0; i < by_len.size(); i++) by_len[i] = i;
				std::stable_sort(by_len.begin(), by_len.end(), [&](size_t a, size_t b) { return qp[a].length < qp[b].length; });
				for (size_t b0 = 0; b0 < by_len.size(); b0 += qblock) {
					const size_t nb = std::min(qblock, by_len.size() - b0);
					size_t lo = pts.size(), hi = 0;
					std::vector<uint32_t> q_slots;
					std::vector<size_t> members;
					for (size_t j = 0; j < nb; j++) {
						const size_t qi = by_len[b0 + j];
						if (win_start[qi] >= win_end[qi]) continue;
						lo = std::min(lo, win_start[qi]);
						hi = std::max(hi, win_end[qi]);
						q_slots.push_back(qp[qi].slot);
						members.push_back(qi);
					}
					if (members.empty()) continue;
					std::vector<uint32_t> window;
					for (size_t i = lo; i < hi; i++) window.push_back(pts[i]->slot);
					if (members.size() == 1 && !both_strands) {          // pred->close / similarity, one query
						std::vector<uint8_t> close;
						std::vector<double> sim;
						pred.search(dset, window, qset, q_slots[0], close, sim);
						note_kernel();
						const size_t before = hits[members[0]].size();
						for (size_t i = win_start[members[0]]; i < win_end[members[0]]; i++)
							if (close[i - lo]) hits[members[0]].push_back(Hit{i, sim[i - lo], 0, 0.0, std::string()});
						num_pred_pos += hits[members[0]].size() - before;
						cut_top(hits[members[0]], top);
						continue;
					}
					// the block in one pass over the union window, each member's own window given: only its close pairs come back
					std::vector<uint64_t> wl(members.size()), wh(members.size());
					for (size_t j = 0; j < members.size(); j++) { wl[j] = win_start[members[j]] - lo; wh[j] = win_end[members[j]] - lo; }
					std::vector<uint32_t> idx;
					std::vector<double> sim;
					std::vector<uint64_t> counts;
					std::vector<uint8_t> strand;
					const std::vector<uint64_t> offsets = both_strands ? pred.search_pairs_strands(dset, window, qset, q_slots, wl, wh, idx, sim, strand)
					                                      : top ? pred.search_pairs_top(dset, window, qset, q_slots, wl, wh, (uint32_t)std::min<size_t>(top, 0xffffffffu), idx, sim, &counts)
					                                          : pred.search_pairs(dset, window, qset, q_slots, wl, wh, idx, sim);
					note_kernel();
					for (size_t j = 0; j < members.size(); j++) num_pred_pos += top ? counts[j] : offsets[j + 1] - offsets[j];
					for (size_t j = 0; j < members.size(); j++)
						for (uint64_t p = offsets[j]; p < offsets[j + 1]; p++) hits[members[j]].push_back(Hit{lo + idx[p], sim[p], both_strands ? strand[p] : (uint8_t)0, 0.0, std::string()});
				}
				if (align) {          // --align: the step's reported pairs in one call, over the strings of the two chunks; sequence 1 = the query (reversed for a `-` hit)
					std::vector<std::string> text;
					std::vector<uint32_t> first, second;
					std::vector<long> q_at(2 * qp.size(), -1), d_at(pts.size(), -1);          // where a query (by strand) / an entry sits in `text`
					std::vector<Hit*> listed;
					for (size_t qi = 0; qi < qp.size(); qi++)
						for (Hit& h : hits[qi]) {
							if (!(h.sim > 0)) continue;
							long& qa = q_at[2 * qi + (h.strand ? 1 : 0)];
							if (qa < 0) { qa = (long)text.size(); text.push_back(h.strand ? msc::reverse_complement(queries[qo + qp[qi].slot].seq) : queries[qo + qp[qi].slot].seq); }
							long& da = d_at[h.cand];
							if (da < 0) { da = (long)text.size(); text.push_back(db[d0 + pts[h.cand]->slot].seq); }
							first.push_back((uint32_t)qa);
							second.push_back((uint32_t)da);
							listed.push_back(&h);
						}
					const std::vector<double> identity = align_band ? msc::align_pairs_long_auto(ctx, text, first, second, first_band).identity : msc::align_pairs_long(ctx, text, first, second).identity;
					note_kernel();
					for (size_t i = 0; i < listed.size(); i++) listed[i]->aln = identity[i];
					if (cigar) {          // --cigar: the listed pairs within msc_align_pairs_trace's limit in one more call; the others print *
						std::vector<uint32_t> short_first, short_second;
						std::vector<Hit*> traced;
						for (size_t i = 0; i < listed.size(); i++) {
							listed[i]->cigar = "*";
							if (text[first[i]].size() > 32767 || text[second[i]].size() > 32767) continue;
							short_first.push_back(first[i]);
							short_second.push_back(second[i]);
							traced.push_back(listed[i]);
						}
						const msc::Traces tr = msc::align_pairs_trace(ctx, text, short_first, short_second);
						note_kernel();
						for (size_t i = 0; i < traced.size(); i++) traced[i]->cigar = tr.cigar(i);
					}
				}
				if (top) {          // the chunk's survivors behind those of the chunks before, cut again: ties stay with the earlier chunk
					for (size_t qi = 0; qi < qp.size(); qi++) {
						for (const Hit& h : hits[qi]) best[qi].push_back(Surv{dchunk, h.cand, h.sim, pts[h.cand]->header, h.aln, h.cigar});
						cut_top(best[qi], top);
					}
					continue;
				}
				for (size_t qi = 0; qi < qp.size(); qi++) {
					const Pt& query = qp[qi];
					for (const Hit& h : hits[qi]) {
						if (h.sim > 0) {
							if (format) out << format_header(query.header) << delim << format_header(pts[h.cand]->header) << delim << 100 * h.sim;
							else out << query.header << delim << pts[h.cand]->header << delim << 100 * h.sim;
							if (both_strands) out << delim << (h.strand ? '-' : '+');
							if (align) out << delim << 100 * h.aln;
							if (cigar) out << delim << h.cigar;
							out << std::endl;
						}
					}
				}
			}
			if (top) {          // the lines of the query chunk, in the order they have without the flag: database chunk, query, window position
				std::vector<size_t> at(qp.size(), 0);
				for (size_t dc = 0; dc < n_dchunks; dc++)
					for (size_t qi = 0; qi < qp.size(); qi++)
						for (; at[qi] < best[qi].size() && best[qi][at[qi]].chunk == dc; at[qi]++) {
							const Surv& h = best[qi][at[qi]];
							if (!(h.sim > 0)) continue;
							if (format) out << format_header(qp[qi].header) << delim << format_header(h.header) << delim << 100 * h.sim;
							else out << qp[qi].header << delim << h.header << delim << 100 * h.sim;
							if (align) out << delim << 100 * h.aln;
							if (cigar) out << delim << h.cigar;
							out << std::endl;
						}
			}
		}
		std::cout << "# of predicted positive: " << num_pred_pos << std::endl;
		for (const auto& kn : kernels) std::fprintf(stderr, "kernel: %s\n", kn.c_str());
	} catch (const msc::Error& e) {
		std::fprintf(stderr, "msc error %d: %s\n", e.code, e.what());
		return 3;
	}
	return 0;
}
