// query_side_check.hip -- the queries' side of the Q x M pass (msc_pair_gemm.hip) alone: the per-block launchers (msc_launch_kb_gather, msc_launch_hot_list,
// msc_launch_pair_gemm_queries) against the grouped launcher (msc_launch_query_group) on random presence bits and random lists of large bins. Compared: qT, anib,
// hot_ptr byte for byte, the hot entries sorted within a bucket (their order comes from atomics). Then both are timed.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../meshclust2_amd/csrc query_side_check.hip -o query_side_check && ./query_side_check [rounds]
#include "../../meshclust2_amd/csrc/msc_pair_gemm.hip"
#include "../../meshclust2_amd/csrc/msc_multi_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

static uint64_t mixh(uint64_t x) { x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull; return x ^ (x >> 31); }

struct Set {
	uint64_t nbins; uint32_t slots, fold, pitch;
	uint8_t *kb = nullptr, *kbf = nullptr;
	uint32_t *x = nullptr, *mb_n = nullptr;
	uint2* mb = nullptr;
	std::vector<uint32_t> mb_n_host;
};

// `per` random bins per slot; lists of `len(slot)` random large bins (len 0 everywhere: no hot list)
static Set make_set(uint64_t nbins, uint32_t slots, uint32_t fold, uint32_t per, uint32_t max_len) {
	Set s; s.nbins = nbins; s.slots = slots; s.fold = fold; s.pitch = 6;
	const uint64_t blocks = (slots + 31) / 32, bytes = blocks * msc_kb_block_bytes(nbins);
	std::vector<uint8_t> h(bytes, 0);
	for (uint32_t sl = 0; sl < slots; sl++)
		for (uint32_t j = 0; j < per; j++) {
			const uint64_t bin = mixh((uint64_t)sl * 4096 + j) % nbins, off = msc_kb_offset(sl, bin, nbins);
			uint16_t hw; memcpy(&hw, &h[off], 2); hw |= (uint16_t)(1u << (bin & 15)); memcpy(&h[off], &hw, 2);
		}
	CK(hipMalloc(&s.kb, bytes)); CK(hipMemcpy(s.kb, h.data(), bytes, hipMemcpyHostToDevice));
	if (fold > 1) {
		CK(hipMalloc(&s.kbf, blocks * msc_kb_block_bytes(nbins / fold))); CK(hipMemset(s.kbf, 0, blocks * msc_kb_block_bytes(nbins / fold)));
		CK(hipMalloc(&s.x, blocks * 32 * 4));
		CK(msc_launch_kb_fold(0, nbins, fold, s.kb, s.kbf, s.x, 0, slots));
	}
	std::vector<uint2> mb((size_t)slots * s.pitch, make_uint2(0, 0));
	s.mb_n_host.assign(slots, 0);
	for (uint32_t sl = 0; sl < slots && max_len; sl++) {
		const uint32_t n = (uint32_t)(mixh(sl ^ 0xabcdefull) % (max_len + 3));          // (now and then longer than the pitch: the kernels clip)
		s.mb_n_host[sl] = n;
		for (uint32_t j = 0; j < std::min(n, s.pitch); j++) mb[(size_t)sl * s.pitch + j] = make_uint2((uint32_t)(mixh((uint64_t)sl * 977 + j + 5) % nbins), 2 + (uint32_t)(mixh(sl + j) % 400));
	}
	CK(hipMalloc(&s.mb, mb.size() * 8)); CK(hipMemcpy(s.mb, mb.data(), mb.size() * 8, hipMemcpyHostToDevice));
	CK(hipMalloc(&s.mb_n, slots * 4)); CK(hipMemcpy(s.mb_n, s.mb_n_host.data(), slots * 4, hipMemcpyHostToDevice));
	CK(hipDeviceSynchronize());
	return s;
}
static void free_set(Set& s) { for (void* p : {(void*)s.kb, (void*)s.kbf, (void*)s.x, (void*)s.mb_n, (void*)s.mb}) if (p) CK(hipFree(p)); }

// n_blocks blocks of 128 query slots (the last one n_q_last), per block and grouped; compare unless timing_only; returns mismatches
static int run_case(const char* what, Set& s, const std::vector<uint32_t>& q_slots, uint32_t n_blocks, uint32_t n_q_last, int rounds, bool compare) {
	const uint64_t nbins = s.nbins, nbins_f = s.fold > 1 ? nbins / s.fold : nbins;
	const uint32_t nsteps = (uint32_t)(nbins_f / 128);
	std::vector<MscGroupBlock> gb(n_blocks);
	std::vector<uint64_t> n_hot(n_blocks, 0);
	for (uint32_t j = 0; j < n_blocks; j++) {
		const uint32_t nq = j + 1 == n_blocks ? n_q_last : 128;
		for (uint32_t r = 0; r < nq; r++) n_hot[j] += std::min(s.mb_n_host[q_slots[128 * j + r]], s.pitch);
		gb[j] = MscGroupBlock{true, s.fold > 1 ? s.fold : 0, n_hot[j]};
	}
	std::vector<MscQueryGroup> groups;
	msc_query_groups(gb, nbins, n_blocks, ~0ull, groups);
	if (groups.size() != 1 || groups[0].n != n_blocks) { fprintf(stderr, "%s: the blocks did not form one group\n", what); return 1; }
	const MscQueryGroup G = groups[0];
	uint32_t* dq; CK(hipMalloc(&dq, q_slots.size() * 4)); CK(hipMemcpy(dq, q_slots.data(), q_slots.size() * 4, hipMemcpyHostToDevice));
	uint8_t *arena, *ref;          // ref: the per-block images in the arena's own layout
	CK(hipMalloc(&arena, G.bytes)); CK(hipMalloc(&ref, G.bytes));
	CK(hipMemset(arena, 0xa5, G.bytes)); CK(hipMemset(ref, 0xa5, G.bytes));
	auto per_block = [&] {
		for (uint32_t j = 0; j < n_blocks; j++) {
			const uint32_t nq = j + 1 == n_blocks ? n_q_last : 128;
			uint8_t *qT = ref + G.qt_off + j * G.qt_stride, *anib = ref + G.anib_off + j * G.anib_stride;
			void* hot = ref + G.hot_off + j * G.hot_stride * 8;
			uint32_t *ptr = (uint32_t*)(ref + G.ptr_off) + j * G.idx_stride, *cur = (uint32_t*)(ref + G.cursor_off) + j * G.idx_stride, *cnt = (uint32_t*)(ref + G.cnt_off) + j * G.idx_stride;
			if (s.fold > 1) {
				CK(msc_launch_kb_gather(0, nbins, s.kb, dq + 128 * j, nq, 128, qT, nullptr));
				CK(msc_launch_kb_gather(0, nbins_f, s.kbf, dq + 128 * j, nq, 128, nullptr, anib));
				CK(msc_launch_hot_list(0, nbins, s.fold, s.mb, s.mb_n, s.pitch, dq + 128 * j, nq, 128, qT, n_hot[j], hot, ptr, cur, cnt));
			} else
				CK(msc_launch_pair_gemm_queries(0, nbins, s.kb, s.mb, s.mb_n, s.pitch, dq + 128 * j, nq, 128, qT, n_hot[j], hot, ptr, cur, cnt, anib));
		}
	};
	auto grouped = [&] {
		CK(msc_launch_query_group(0, nbins, G.fold, s.kb, s.kbf, s.mb, s.mb_n, s.pitch, dq, n_blocks, n_q_last, arena + G.qt_off, G.qt_stride, arena + G.anib_off, G.anib_stride,
		                          G.hot_stride, arena + G.hot_off, (uint32_t*)(arena + G.ptr_off), (uint32_t*)(arena + G.cursor_off), (uint32_t*)(arena + G.cnt_off), G.idx_stride));
	};
	per_block(); grouped();
	CK(hipDeviceSynchronize());
	int bad = 0;
	if (compare) {
		std::vector<uint8_t> a(G.bytes), b(G.bytes);
		CK(hipMemcpy(a.data(), arena, G.bytes, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), ref, G.bytes, hipMemcpyDeviceToHost));
		uint64_t bad_qt = 0, bad_anib = 0, bad_ptr = 0, bad_hot = 0;
		for (uint64_t i = G.qt_off; i < G.anib_off; i++) bad_qt += a[i] != b[i];
		for (uint64_t i = G.anib_off; i < G.hot_off; i++) bad_anib += a[i] != b[i];
		for (uint32_t j = 0; j < n_blocks && G.hot_stride; j++) {
			if (!n_hot[j]) continue;          // (the per-block path builds no list for such a block)
			const uint32_t *pa = (const uint32_t*)(a.data() + G.ptr_off) + j * G.idx_stride, *pb = (const uint32_t*)(b.data() + G.ptr_off) + j * G.idx_stride;
			for (uint32_t i = 0; i <= nsteps; i++) bad_ptr += pa[i] != pb[i];
			if (pb[nsteps] != n_hot[j]) bad_ptr++;
			std::vector<uint64_t> ea(n_hot[j]), eb(n_hot[j]);
			memcpy(ea.data(), a.data() + G.hot_off + j * G.hot_stride * 8, n_hot[j] * 8); memcpy(eb.data(), b.data() + G.hot_off + j * G.hot_stride * 8, n_hot[j] * 8);
			for (uint32_t i = 0; i < nsteps && !bad_ptr; i++) { std::sort(ea.begin() + pb[i], ea.begin() + pb[i + 1]); std::sort(eb.begin() + pb[i], eb.begin() + pb[i + 1]); }
			for (uint64_t i = 0; i < n_hot[j]; i++) bad_hot += ea[i] != eb[i];
		}
		bad = (int)std::min<uint64_t>(bad_qt + bad_anib + bad_ptr + bad_hot, 1u << 30);
		printf("%-58s qT %llu anib %llu ptr %llu hot %llu bytes / words / entries differ (n_hot %llu %llu ..)%s\n", what, (unsigned long long)bad_qt, (unsigned long long)bad_anib,
		       (unsigned long long)bad_ptr, (unsigned long long)bad_hot, (unsigned long long)n_hot[0], (unsigned long long)(n_blocks > 1 ? n_hot[1] : 0), bad ? "  <-- MISMATCH" : "");
	}
	if (rounds > 0 && !bad) {
		hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
		auto timed = [&](auto&& launch) { CK(hipEventRecord(e0)); launch(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms, e0, e1)); return ms; };
		std::vector<float> tp, tg;
		for (int r = 0; r < rounds; r++) { tp.push_back(timed(per_block)); tg.push_back(timed(grouped)); }
		std::sort(tp.begin(), tp.end()); std::sort(tg.begin(), tg.end());
		const double moved = (double)n_blocks * (nbins / 8 * 128 + (s.fold > 1 ? nbins_f / 8 * 128 : 0) + nbins * 32 + nbins_f * 64);          // mirror rows in, images out
		printf("%-58s per block %.1f us a block, grouped %.1f us a block (medians of %d); grouped moves %.1f MB = %.3f of 8 TB/s\n", what, 1e3 * tp[rounds / 2] / n_blocks,
		       1e3 * tg[rounds / 2] / n_blocks, rounds, moved / 1e6, moved / (1e-3 * tg[rounds / 2]) / 8e12);
		CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
	}
	CK(hipFree(dq)); CK(hipFree(arena)); CK(hipFree(ref));
	return bad;
}

int main(int argc, char** argv) {
	const int rounds = argc > 1 ? atoi(argv[1]) : 7;
	int bad = 0;
	for (int k : {8, 9})
		for (uint32_t fold : {1u, 16u})
			for (uint32_t max_len : {0u, 6u}) {
				Set s = make_set(1ull << (2 * k), 1024, fold, 990, max_len);
				std::vector<uint32_t> slots(1024);
				std::iota(slots.begin(), slots.end(), 0u);
				for (uint32_t i = 1023; i > 0; i--) std::swap(slots[i], slots[mixh(i + 31 * k) % (i + 1)]);          // shuffled
				slots.resize(384);
				char what[96];
				snprintf(what, sizeof what, "k %d fold %2u lists up to %u, 3 x 128 shuffled slots", k, fold, max_len);
				bad += run_case(what, s, slots, 3, 128, 0, true) != 0;
				snprintf(what, sizeof what, "k %d fold %2u lists up to %u, 128 + 128 + 77 shuffled slots", k, fold, max_len);
				bad += run_case(what, s, slots, 3, 77, 0, true) != 0;
				free_set(s);
			}
	if (bad) { printf("query side check FAILED: %d cases\n", bad); return 1; }
	printf("query side check ok\n");
	// the benchmark's shape: 32 blocks of 128 consecutive slots at k = 9, folded x 16 and not; then shuffled slots
	for (uint32_t fold : {16u, 1u})
		for (int shuffled = 0; shuffled < 2; shuffled++) {
			Set s = make_set(262144, 4096, fold, 990, 6);
			std::vector<uint32_t> slots(4096);
			std::iota(slots.begin(), slots.end(), 0u);
			if (shuffled) for (uint32_t i = 4095; i > 0; i--) std::swap(slots[i], slots[mixh(i) % (i + 1)]);
			char what[96];
			snprintf(what, sizeof what, "k 9 fold %2u, %u x 128 %s slots", fold, fold > 1 ? 32u : 16u, shuffled ? "shuffled" : "consecutive");
			bad += run_case(what, s, slots, fold > 1 ? 32 : 16, 128, rounds, false) != 0;
			free_set(s);
		}
	return bad ? 1 : 0;
}
