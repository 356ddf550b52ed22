"""msc_hist_revcomp_batch, msc_search_pairs_strands and msc_search_pairs_fetch_strands through the public layers, without a device: the header
declares them with the documented signatures and states their rules, the built library exports them, the ctypes table and the api classes carry
them, a call without a context is MSC_ERR_INVALID_ARG, and msc_fastcar names --both-strands in its usage line and refuses it beside --top."""
import ctypes as C
import os
import re
import subprocess

import pytest

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "msc_hist_revcomp_batch": """int msc_hist_revcomp_batch(msc_ctx* ctx, msc_hist_set* dst, const uint32_t* dst_slots,
                           const msc_hist_set* src, const uint32_t* src_slots, uint64_t n);""",
    "msc_search_pairs_strands": """int msc_search_pairs_strands(msc_ctx* ctx, const msc_model* cls, const msc_model* reg,
                             const msc_hist_set* db, const uint32_t* db_slots, uint64_t m,
                             const msc_hist_set* qset, const uint32_t* q_slots, uint64_t n_q,
                             const uint64_t* win_lo, const uint64_t* win_hi, uint64_t* offsets, msc_pairs_info* info);""",
    "msc_search_pairs_fetch_strands": "int msc_search_pairs_fetch_strands(msc_ctx* ctx, uint64_t first, uint64_t n, uint8_t* strand);",
}


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def _header():
    return open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_declares_the_signature(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\([^;]*\)\s*;" % name, text)
    assert m, name + " is not declared"
    assert _tokens(m.group(0)) == _tokens(SIGNATURES[name]), m.group(0)


def test_abi_version_and_pairs_info_keep_their_shape():
    text = _header()
    assert re.search(r"#define\s+MSC_ABI_VERSION\s+1\b", text)
    assert C.sizeof(_capi.PairsInfo) == 24


def test_header_comments_state_the_rules():
    text = _header()
    op = text[:text.index("int msc_hist_revcomp_batch")].rsplit("/*", 1)[1]
    for words in ("fastcar/FC_Runner.cpp:426-471", "4^(k-1-j)", "one_mers'[i] = one_mers[3 - i]", "exact copy", "tile prefixes", "MSC_ERR_INVALID_ARG", "MSC_ERR_OOM"):
        assert words in op, words
    call = text[:text.index("int msc_search_pairs_strands")].rsplit("/*", 1)[1]
    for words in ("fastcar/FC_Runner.cpp:426-471", "4^(k-1-j)", "one_mers reversed", "a tie goes to forward", "n_q slots", "batches", "MSC_ERR_UNSUPPORTED", "MSC_ERR_OOM"):
        assert words in call, words


def test_library_exports_them_and_the_table_carries_them():
    lib = _capi.load_library()
    for name, n_args in (("msc_hist_revcomp_batch", 6), ("msc_search_pairs_strands", 13), ("msc_search_pairs_fetch_strands", 4)):
        assert hasattr(lib, name), name
        restype, argtypes = _capi.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    offsets = (C.c_uint64 * 2)()
    slots = (C.c_uint32 * 1)()
    strand = (C.c_uint8 * 1)()
    assert lib.msc_hist_revcomp_batch(None, None, slots, None, slots, 1) == -1          # MSC_ERR_INVALID_ARG
    assert lib.msc_search_pairs_strands(None, None, None, None, None, 0, None, None, 0, None, None, offsets, None) == -1
    assert lib.msc_search_pairs_fetch_strands(None, 0, 0, strand) == -1


def test_api_has_the_methods():
    assert callable(getattr(api.HistogramSet, "revcomp_batch", None))
    assert callable(getattr(api.Predictor, "search_pairs_strands", None))


def _fastcar():
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    exe = os.path.join(host, "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    return exe


def test_fastcar_usage_names_the_flag():
    r = subprocess.run([_fastcar()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 1 and b"usage:" in r.stdout and b"[--both-strands]" in r.stdout, r.stdout


def test_fastcar_refuses_the_flag_beside_top():
    r = subprocess.run([_fastcar(), "db.fa", "--query", "q.fa", "--recover", "w.txt", "--both-strands", "--top", "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=60)
    assert r.returncode == 1 and b"--both-strands" in r.stdout and b"--top" in r.stdout, r.stdout
