"""msc_search_pairs_top through the public layers, without a device: the header declares it with the documented signature, the built library
exports it, the ctypes table and api.Predictor carry it, a call without a context is MSC_ERR_INVALID_ARG, and msc_fastcar names --top in its
usage line."""
import ctypes as C
import os
import re
import subprocess

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURE = """int msc_search_pairs_top(msc_ctx* ctx, const msc_model* cls, const msc_model* reg,
                         const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
                         const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q,
                         const uint64_t* win_lo, const uint64_t* win_hi, uint32_t top_n,
                         uint64_t* offsets, uint64_t* close_counts, msc_pairs_info* info);"""


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def test_header_declares_the_signature():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+msc_search_pairs_top\s*\([^;]*\)\s*;", text)
    assert m, "msc_search_pairs_top is not declared"
    assert _tokens(m.group(0)) == _tokens(SIGNATURE), m.group(0)
    # msc_pairs_info keeps its layout: existing callers pass the current struct
    assert C.sizeof(_capi.PairsInfo) == 24
    assert re.search(r"typedef struct \{\s*uint64_t n_pairs;\s*int32_t\s+route;\s*int32_t\s+pad_;\s*uint64_t fp64_pairs;\s*\} msc_pairs_info;", text)


def test_header_comment_states_the_rule():
    text = open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()
    comment = text[:text.index("int msc_search_pairs_top")].rsplit("/*", 1)[1]
    for words in ("fastcar/FC_Runner.cpp:426-471", "-0.0 == 0.0", "lower candidate index", "ascending i", "top_n == 0", "close_counts"):
        assert words in comment, words


def test_library_exports_it_and_the_table_carries_it():
    lib = _capi.load_library()
    assert hasattr(lib, "msc_search_pairs_top")
    restype, argtypes = _capi.PROTOTYPES["msc_search_pairs_top"]
    assert restype is C.c_int and len(argtypes) == 15 and argtypes[11] is C.c_uint32
    offsets = (C.c_uint64 * 2)()
    assert lib.msc_search_pairs_top(None, None, None, None, None, 0, None, None, 0, None, None, 1, offsets, None, None) == -1          # MSC_ERR_INVALID_ARG


def test_predictor_has_the_method():
    assert callable(getattr(api.Predictor, "search_pairs_top", None))


def test_fastcar_usage_names_the_flag():
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    exe = os.path.join(host, "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 1 and b"usage:" in r.stdout and b"[--top N]" in r.stdout, r.stdout
