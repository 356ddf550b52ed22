"""k_hist_canonical's tiling (meshclust2_amd/csrc/msc_canonical.hip over msc_revcomp_plan.h) as a stand-alone host program: for every dense shape the
tiled kernel serves, the free bits of a tile are closed under the reverse-complement map (fs == fd), so tiles pair up; the program then runs the
kernel's item loop thread by thread IN PLACE -- both tiles of a pair read first, each turned through the tile buffer for the other, both written --
and compares with D[b] + D[rc(b)] - 1 applied element by element, every element written exactly once (the data up to 16 MiB a slot, the plan
alone for larger ones). Built with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meshclust2_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cstring>
#include "msc_revcomp_plan.h"
template <typename T> int run(int k, bool plan_only) {
	const int dtype = sizeof(T) * 8;
	MscLayout L = msc_make_layout(k, dtype);
	if (L.slot_bytes <= 64 * 1024) return 0;
	if (L.nbins != L.padded_bins) { printf("k %d dt %d not whole\n", k, dtype); return 1; }
	MscRcPlan p = msc_rc_plan(L, k);
	if (!msc_rc_plan_fits(p, L) || p.fs != p.fd) { printf("k %d dt %d: fits %d fs %llx fd %llx\n", k, dtype, (int)msc_rc_plan_fits(p, L), (unsigned long long)p.fs, (unsigned long long)p.fd); return 1; }
	if (plan_only) return 0;
	const uint32_t E = L.E, lgE = msc_log2u(E);
	const uint32_t maxchunks = (256u / sizeof(T)) * (256u / sizeof(T)) / E;
	const uint32_t BLOCK = maxchunks / 4 > 256 ? maxchunks / 4 : 256;
	const uint32_t threads = std::min<uint32_t>(BLOCK, (1u << p.f_bits) / E);
	const uint32_t per = ((1u << p.f_bits) / E) / threads;
	std::vector<T> src(L.padded_bins), dst(L.padded_bins), ref(L.padded_bins);
	for (auto& v : src) v = (T)(1 + rand() % 200);
	for (uint64_t ph = 0; ph < L.padded_bins; ph++) ref[ph] = (T)(src[ph] + src[msc_rc_phys(ph, k, E, L.R)] - 1);
	const uint64_t z = msc_rc_phys(0, k, E, L.R);
	std::vector<uint32_t> delta(E);
	for (uint32_t j = 0; j < E; j++) delta[j] = msc_rc_swizzle((uint32_t)msc_bits_extract(msc_rc_phys(j, k, E, L.R) ^ z, p.fd), p, lgE);
	const uint32_t tiles_bits = p.n_bits - p.f_bits;
	const uint64_t all = (1ull << p.n_bits) - 1;
	std::vector<T> tile(1u << p.f_bits);
	std::vector<char> written(L.padded_bins, 0);
	dst = src;   // in place
	for (uint64_t g = 0; g < (1ull << tiles_bits); g++) {
		const uint64_t a_base = msc_bits_deposit(g, all & ~p.fd);
		const uint64_t b_base = msc_rc_phys(a_base, k, E, L.R) & ~p.fd;
		if (b_base < a_base) continue;
		const bool two = a_base != b_base;
		std::vector<T> va((size_t)threads * per * E), vb(va.size());
		auto off = [&](uint32_t t, uint32_t i) { return (uint32_t)msc_bits_deposit((t + i * threads) * E, p.fd); };
		for (uint32_t t = 0; t < threads; t++) for (uint32_t i = 0; i < per; i++) for (uint32_t j = 0; j < E; j++) {
			va[((size_t)t * per + i) * E + j] = dst[a_base + off(t, i) + j];
			vb[((size_t)t * per + i) * E + j] = dst[b_base + off(t, i) + j];
		}
		for (int half = 0; half < 2; half++) {
			if (half && !two) break;
			auto& own = half ? vb : va; auto& other = half ? va : vb;
			for (uint32_t t = 0; t < threads; t++) for (uint32_t i = 0; i < per; i++) {
				const uint32_t at = msc_rc_swizzle((uint32_t)msc_bits_extract(msc_rc_phys((z & ~p.fd) | off(t, i), k, E, L.R), p.fd), p, lgE);
				for (uint32_t j = 0; j < E; j++) tile.at(at ^ delta[j]) = other[((size_t)t * per + i) * E + j];
			}
			for (uint32_t t = 0; t < threads; t++) for (uint32_t i = 0; i < per; i++) {
				const uint32_t c = (t + i * threads) * E, ao = msc_rc_swizzle(c, p, lgE);
				for (uint32_t j = 0; j < E; j++) {
					const uint64_t w = (half ? b_base : a_base) + off(t, i) + j;
					if (w >= L.padded_bins) { printf("destination k=%d u%d\n", k, dtype); return 1; }
					dst[w] = (T)(own[((size_t)t * per + i) * E + j] + tile.at(ao + j) - 1);
					written[w]++;
				}
			}
		}
	}
	uint64_t bad = 0;
	for (uint64_t ph = 0; ph < L.padded_bins; ph++) if (dst[ph] != ref[ph] || written[ph] != 1) bad++;
	if (bad) printf("tiles k=%d u%d: %llu elements\n", k, dtype, (unsigned long long)bad);
	return bad != 0;
}
int main() {
	int r = 0;
	for (int k = 6; k <= 13; k++) {          // (every dense shape the tiled kernel serves: the plan; the data up to 16 MiB a slot)
		r |= run<uint8_t>(k, k > 12); r |= run<uint16_t>(k, k > 11); r |= run<uint32_t>(k, k > 10); r |= run<uint64_t>(k, k > 10);
	}
	printf(r ? "FAIL\n" : "ALL OK\n");
	return r;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("canonical_tiles")
    src = d / "canonical_tiles.cpp"
    src.write_text(PROGRAM)
    exe = str(d / "canonical_tiles")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", exe])
    return exe


def test_the_paired_tiling_in_place_on_the_host(program):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith(b"ALL OK"), r.stdout.decode(errors="replace")[-2000:]
