"""msc_score_pair_list through the public layers, without a device: the header declares it with the documented signature and states its
contract, the built library exports it, the ctypes table, api.py and the C++ host mirror carry it, a call without a context is
MSC_ERR_INVALID_ARG, and the host bookkeeping of the call (grouping by second slot, chunking, scatter back: csrc/msc_pair_groups.h) holds
against a brute-force map in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURE = """int msc_score_pair_list(msc_ctx* ctx, const msc_model* model,
                        const msc_hist_set* a_set, const uint32_t* a_slots,
                        const msc_hist_set* b_set, const uint32_t* b_slots, uint64_t n, int order,
                        uint64_t feat_mask, double* raw_out,
                        double* singles_out, double* combos_out, double* sum_out, double* csum_out, uint8_t* close_out);"""


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def test_header_declares_the_signature():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+msc_score_pair_list\s*\([^;]*\)\s*;", text)
    assert m, "msc_score_pair_list is not declared"
    assert _tokens(m.group(0)) == _tokens(SIGNATURE), m.group(0)
    assert re.search(r"#define\s+MSC_ABI_VERSION\s+1\b", text)          # the change is additive


def test_header_comment_states_the_contract():
    text = open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()
    comment = text[:text.index("int msc_score_pair_list")].rsplit("/*", 1)[1]
    for words in ("predict/FeatureSelector.cpp:23-33", "predict/Predictor.cpp:876-985", "caller's order", "bit", "k_pair_sparse_wl_pairs", " per query",
                  "MSC_ERR_ZERO_LENGTH", "no length window"):
        assert words in comment, words


def test_library_exports_it_and_the_table_carries_it():
    lib = _capi.load_library()
    assert hasattr(lib, "msc_score_pair_list")
    restype, argtypes = _capi.PROTOTYPES["msc_score_pair_list"]
    assert restype is C.c_int and len(argtypes) == 15 and argtypes[6] is C.c_uint64 and argtypes[8] is C.c_uint64
    raw = (C.c_double * 4)()
    assert lib.msc_score_pair_list(None, None, None, None, None, None, 1, 0, 1 << 2, raw, None, None, None, None, None) == -1          # MSC_ERR_INVALID_ARG
    assert lib.msc_abi_version() == 1


def test_every_declared_symbol_is_still_exported():
    from tests.test_abi_cpu import test_library_exports_every_declared_symbol
    test_library_exports_every_declared_symbol()


def test_api_has_the_three_entry_points():
    assert callable(getattr(api, "score_pair_list", None))
    assert callable(getattr(api.Feature, "compute_pairs", None))
    assert callable(getattr(api.Predictor, "score_pairs", None))


SNIPPET = r"""
#include "meshclust2_host.hpp"
int use(msc::Context& ctx, msc::PointSet& a, msc::PointSet& b, const msc::Feature& f, const msc::Predictor& p) {
	std::vector<uint32_t> as(3, 0), bs(3, 1);
	std::vector<double> combos, sums, sim;
	std::vector<uint8_t> close;
	std::vector<double> singles = f.compute_pairs(a, as, b, bs, MSC_ORDER_QUERY_FIRST, &combos, &sums);
	p.score_pairs(a, as, b, bs, close, sim);
	(void)ctx;
	return (int)(singles.size() + combos.size() + sums.size() + close.size() + sim.size());
}
int main() { return 0; }
"""


def test_cpp_host_mirror_carries_the_pair_list_calls(tmp_path):
    src = tmp_path / "pair_list_snippet.cpp"
    src.write_text(SNIPPET)
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "meshclust2_amd", "host"), "-c", str(src), "-o", str(tmp_path / "snippet.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()


def test_pair_grouping_chunking_and_scatter_under_sanitizers(tmp_path):
    exe = tmp_path / "pair_groups_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "pair_groups_check.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"pair groups ok" in r.stdout, r.stdout.decode()
