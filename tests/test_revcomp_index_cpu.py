"""msc_rc_bin (meshclust2_amd/csrc/msc_revcomp.h), the one index function the reverse-complement kernels and the host share, as a stand-alone host
program: every bin of k = 1 .. 8 against the index of the reverse-complemented k-mer string, the involution, 10^5 random bins at k = 13 and 15
against a digit loop, palindromes. The same program emulates k_hist_revcomp's tiling (msc_revcomp_plan.h) on the host for every dense shape the
tiled kernel serves up to 16 MiB a slot, against the permutation applied bin by bin (the plan alone for the larger ones). Built with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meshclust2_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "msc_revcomp_plan.h"

static uint64_t index_of(const std::string& s) {
	uint64_t b = 0;
	for (char c : s) b = b * 4 + (c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3);
	return b;
}
static std::string kmer_of(uint64_t b, int k) {
	std::string s(k, 'A');
	for (int i = k - 1; i >= 0; i--) { s[i] = "ACGT"[b & 3]; b >>= 2; }
	return s;
}
static std::string rc_string(const std::string& s) {
	std::string r(s.rbegin(), s.rend());
	for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
	return r;
}
static uint64_t rc_digits(uint64_t b, int k) {
	uint64_t r = 0;
	for (int i = 0; i < k; i++) r |= (3 - ((b >> (2 * i)) & 3)) << (2 * (k - 1 - i));
	return r;
}

template <typename T>
static int tiled(int k, int dtype, bool plan_only) {
	const MscLayout L = msc_make_layout(k, dtype);
	if (L.slot_bytes <= 64 * 1024) return 0;
	const uint32_t E = L.E, lgE = msc_log2u(E);
	const MscRcPlan p = msc_rc_plan(L, k);
	if (L.nbins != L.padded_bins || !msc_rc_plan_fits(p, L)) { printf("plan k=%d u%d\n", k, dtype); return 1; }
	const uint32_t chunks = (1u << p.f_bits) / E, want_block = MSC_RC_MAX_CHUNKS(T) / 4 > 256 ? MSC_RC_MAX_CHUNKS(T) / 4 : 256;
	const uint32_t block = chunks < want_block ? chunks : want_block, per = chunks / block;
	if (per * block != chunks || per > MSC_RC_MAX_CHUNKS(T) / want_block) { printf("chunks per thread k=%d u%d\n", k, dtype); return 1; }
	if (plan_only) return 0;
	std::vector<T> src(L.padded_bins), want(L.padded_bins), dst(L.padded_bins, (T)0xAB), tile(1u << p.f_bits);
	for (uint64_t b = 0; b < L.nbins; b++) src[msc_phys_index(b, L.E, L.R)] = (T)(b * 2654435761u + 7);
	for (uint64_t b = 0; b < L.nbins; b++) want[msc_phys_index(b, L.E, L.R)] = src[msc_phys_index(msc_rc_bin(b, k), L.E, L.R)];
	// what a thread of k_hist_revcomp holds in registers: the same for every tile
	const uint64_t z = msc_rc_phys(0, k, E, L.R), all = (1ull << p.n_bits) - 1;
	std::vector<uint32_t> delta(E), s_off(chunks), at_in(chunks), d_off(chunks), at_out(chunks);
	for (uint32_t j = 0; j < E; j++) delta[j] = msc_rc_swizzle((uint32_t)msc_bits_extract(msc_rc_phys(j, k, E, L.R) ^ z, p.fd), p, lgE);
	for (uint32_t u = 0; u < chunks; u++) {
		const uint32_t c = u * E;
		s_off[u] = (uint32_t)msc_bits_deposit(c, p.fs);
		at_in[u] = msc_rc_swizzle((uint32_t)msc_bits_extract(msc_rc_phys((z & ~p.fs) | s_off[u], k, E, L.R), p.fd), p, lgE);
		d_off[u] = (uint32_t)msc_bits_deposit(c, p.fd);
		at_out[u] = msc_rc_swizzle(c, p, lgE);
	}
	for (uint64_t g = 0; g < (1ull << (p.n_bits - p.f_bits)); g++) {          // the item loop of the kernel, chunk by chunk
		const uint64_t d_base = msc_bits_deposit(g, all & ~p.fd), s_base = msc_rc_phys(d_base, k, E, L.R) & ~p.fs;
		if ((s_base & p.fs) || (d_base & p.fd)) { printf("bases k=%d u%d\n", k, dtype); return 1; }
		for (uint32_t u = 0; u < chunks; u++) {
			const uint64_t s = s_base + s_off[u];
			if (s % E || s + E > L.padded_bins) { printf("source run k=%d u%d\n", k, dtype); return 1; }
			for (uint32_t j = 0; j < E; j++) tile.at(at_in[u] ^ delta[j]) = src[s + j];
		}
		for (uint32_t u = 0; u < chunks; u++) {
			const uint64_t d = d_base + d_off[u];
			if (d % E || d + E > L.padded_bins || at_out[u] % E) { printf("destination run k=%d u%d\n", k, dtype); return 1; }
			for (uint32_t j = 0; j < E; j++) dst[d + j] = tile.at(at_out[u] + j);
		}
	}
	if (memcmp(dst.data(), want.data(), L.slot_bytes)) { printf("tiles k=%d u%d\n", k, dtype); return 1; }
	return 0;
}

int main() {
	int bad = 0;
	for (int k = 1; k <= 8; k++) {
		uint64_t fixed = 0;
		for (uint64_t b = 0; b < (1ull << (2 * k)); b++) {
			const uint64_t r = msc_rc_bin(b, k);
			if (r != index_of(rc_string(kmer_of(b, k)))) { printf("k=%d bin %llu\n", k, (unsigned long long)b); bad = 1; }
			if (msc_rc_bin(r, k) != b) { printf("involution k=%d bin %llu\n", k, (unsigned long long)b); bad = 1; }
			fixed += r == b;
		}
		// a palindrome is fixed by its first half: 4^(k/2) of them for even k, none for odd k
		if (fixed != (k % 2 ? 0 : 1ull << k)) { printf("palindromes k=%d: %llu\n", k, (unsigned long long)fixed); bad = 1; }
	}
	if (msc_rc_bin(index_of("ACGT"), 4) != index_of("ACGT") || msc_rc_bin(index_of("AATT"), 4) != index_of("AATT")) { printf("ACGT / AATT\n"); bad = 1; }
	if (msc_rc_bin(0, 9) != (1ull << 18) - 1 || msc_rc_bin(index_of("AAC"), 3) != index_of("GTT")) { printf("poly-A / AAC\n"); bad = 1; }
	uint64_t x = 0x9E3779B97F4A7C15ull;
	for (int k : {13, 15})
		for (int i = 0; i < 100000; i++) {
			x ^= x << 13; x ^= x >> 7; x ^= x << 17;
			const uint64_t b = x & ((1ull << (2 * k)) - 1), r = msc_rc_bin(b, k);
			if (r != rc_digits(b, k) || msc_rc_bin(r, k) != b) { printf("k=%d bin %llu\n", k, (unsigned long long)b); bad = 1; }
		}
	for (int k = 7; k <= 13; k++) {          // (every dense shape the tiled kernel serves: the plan; the data up to 16 MiB a slot)
		bad |= tiled<uint8_t>(k, 8, k > 12);
		bad |= tiled<uint16_t>(k, 16, k > 11);
		bad |= tiled<uint32_t>(k, 32, k > 10);
		bad |= tiled<uint64_t>(k, 64, k > 10);
	}
	printf(bad ? "FAIL\n" : "ALL OK\n");
	return bad;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("rc_bin")
    src = d / "rc_bin.cpp"
    src.write_text(PROGRAM)
    exe = str(d / "rc_bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", exe])
    return exe


def test_rc_bin_and_the_tiling_on_the_host(program):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith(b"ALL OK"), r.stdout.decode(errors="replace")[-2000:]
