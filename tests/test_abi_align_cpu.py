"""msc_align_pairs through the public layers, without a device: the header declares it with the documented signature and states its rules, the
built library exports it, the ctypes table, api.py and the C++ host mirror carry it, a call without a context is refused cleanly and leaves its
outputs alone, msc_fastcar names [--align] and refuses it beside --canonical before it opens a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURE = """int msc_align_pairs(msc_ctx* ctx,
                    const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                    const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                    int match, int mismatch, int gap_open, int gap_continue,
                    int32_t* score, int32_t* length, int32_t* matches);"""


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def _header():
    return open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()


def test_header_declares_the_signature():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+msc_align_pairs\s*\([^;]*\)\s*;", text)
    assert m, "msc_align_pairs is not declared"
    assert _tokens(m.group(0)) == _tokens(SIGNATURE), m.group(0)
    assert re.search(r"#define\s+MSC_ABI_VERSION\s+1\b", _header())          # the change is additive


def test_header_comment_states_the_rules():
    text = _header()
    comment = text[:text.index("int msc_align_pairs")].rsplit("/* ---", 1)[1]
    for words in ("predict/Feature.cpp:697-718", "utility/GlobAlignE.cpp:123-292", "first is GlobAlignE's seq1", "an N equals an N", "1 .. 32 767", "at most 100",
                  "MSC_ERR_INVALID_ARG", "n_pairs == 0 is MSC_OK", "untouched", "k_align_pairs", "caller's order"):
        assert words in comment, words


def test_design_counts_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = len(set(re.findall(r"\b(msc_\w+)\s*\(", text)))
    m = re.search(r"\((\d+) entry points", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert m and int(m.group(1)) == declared, (m and m.group(1), declared)


def test_library_exports_it_and_the_layers_carry_it():
    lib = _capi.load_library()
    assert hasattr(lib, "msc_align_pairs")
    restype, argtypes = _capi.PROTOTYPES["msc_align_pairs"]
    assert restype is C.c_int and len(argtypes) == 14
    assert argtypes[3] is C.c_uint64 and argtypes[6] is C.c_uint64 and all(argtypes[i] is C.c_int for i in (7, 8, 9, 10))
    out = (C.c_int32 * 1)(-7)
    text, offsets, idx = (C.c_uint8 * 2)(65, 0), (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 1)(0)
    assert lib.msc_align_pairs(None, text, offsets, 1, idx, idx, 1, 1, -1, 2, 1, out, out, out) == -1          # MSC_ERR_INVALID_ARG
    assert out[0] == -7
    assert lib.msc_abi_version() == 1
    mirror = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"inline\s+Alignments\s+align_pairs\s*\(", mirror) and "msc_align_pairs(" in mirror


def test_every_declared_symbol_is_still_exported():
    from tests.test_abi_cpu import test_library_exports_every_declared_symbol
    test_library_exports_every_declared_symbol()


def test_api_align_pairs_raises_cleanly_without_a_device():
    assert callable(getattr(api, "align_pairs", None))
    out = tuple(np.full(2, -7, dtype=np.int32) for _ in range(3))
    with pytest.raises(api.MscError) as e:
        api.align_pairs(None, [b"ACGT", "ACCT"], [0, 1], [1, 1], out=out)
    assert e.value.code == -1 and "Context" in str(e.value)
    assert all((o == -7).all() for o in out)
    with pytest.raises(ValueError):
        api.align_pairs(None, [b"ACGT"], [0, 0], [0])


SNIPPET = r"""
#include "meshclust2_host.hpp"
double use(msc::Context& ctx) {
	std::vector<std::string> seqs(2, "ACGT");
	std::vector<uint32_t> first(1, 0), second(1, 1);
	msc::Alignments a = msc::align_pairs(ctx, seqs, first, second);
	msc::Alignments b = msc::align_pairs(ctx, seqs, first, second, 2, -3, 5, 2);
	return a.identity[0] + b.score[0] + b.length[0] + b.matches[0] + (double)msc::reverse_complement(seqs[0]).size();
}
int main() { return msc::reverse_complement("AACGNTx") == "xANCGTT" ? 0 : 1; }
"""


def test_cpp_host_mirror_carries_the_call(tmp_path):
    src = tmp_path / "align_snippet.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "align_snippet"
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I", host, str(src), "-L", os.path.join(ROOT, "meshclust2_amd"), "-lmeshclust2_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "meshclust2_amd"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert subprocess.run([str(exe)], timeout=60).returncode == 0


def _fastcar():
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    exe = os.path.join(host, "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    return exe


def test_fastcar_names_the_flag_and_refuses_it_beside_canonical():
    r = subprocess.run([_fastcar()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 1 and b"usage:" in r.stdout and b"[--align]" in r.stdout, r.stdout
    # the files do not exist and there may be no device: the refusal comes before either is looked at
    r = subprocess.run([_fastcar(), "db.fa", "--query", "q.fa", "--recover", "w.txt", "--align", "--canonical"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 1 and b"--align" in r.stdout and b"--canonical" in r.stdout and b"msc error" not in r.stdout, r.stdout
