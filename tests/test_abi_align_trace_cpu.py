"""msc_align_pairs_trace and msc_align_pairs_trace_fetch through the public layers, without a device: the header declares them after
msc_align_pairs_long_auto and states the definition, the built library exports them, the ctypes table, api.py and the C++ host mirror carry
them, a call without a context is refused cleanly and leaves its outputs alone, DESIGN.md counts them, has section 4.6h and lists the switch,
msc_fastcar's usage comment describes --cigar."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msc_align_pairs_trace", "msc_align_pairs_trace_fetch")


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def _header():
    return open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()


def _declaration(text, name):
    m = re.search(r"\bint\s+%s\s*\([^;]*\)\s*;" % name, text)
    assert m, name + " is not declared"
    return m


def test_header_declares_them_after_the_long_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    trace, fetch = _declaration(text, NAMES[0]), _declaration(text, NAMES[1])
    assert _declaration(text, "msc_align_pairs_long_auto").start() < trace.start() < fetch.start()
    # msc_align_pairs's arguments, then the offsets of the op list
    plain = _tokens(_declaration(text, "msc_align_pairs").group(0))
    assert _tokens(trace.group(0)) == ["int", NAMES[0]] + plain[2:-2] + _tokens(", uint64_t* op_offsets);")
    assert _tokens(fetch.group(0)) == _tokens("int msc_align_pairs_trace_fetch(msc_ctx* ctx, uint64_t first_word, uint64_t n_words, uint32_t* ops);")
    assert re.search(r"#define\s+MSC_ABI_VERSION\s+1\b", _header())          # the change is additive


def test_header_comment_states_the_definition():
    text = _header()
    comment = text[:text.index("int msc_align_pairs_trace(")].rsplit("/* ---", 1)[1]
    assert "int msc_align_pairs_long_auto(" not in comment          # a block of their own
    for words in ("DESIGN.md 4.6h", "1 .. 32 767", "at most 100", "MSC_ERR_INVALID_ARG", "untouched", "n_pairs == 0 is MSC_OK", "op_offsets[0] = 0", "bit for bit",
                  "match, then", "lower, then upper", "run << 4 | op", "BAM", "7 '='", "8 'X'", "1 'I'", "2 'D'", "is the query", "the reference", "Adjacent runs never share an op",
                  "n_pairs + 1", "until the next msc_align_pairs_trace", "msc_destroy", "past its end", "number `length`", "number `matches`", "match != mismatch", "REAL path",
                  "is `score`", "kAlignTraceBytes", "MSC_ALIGN_TRACE_BYTES=n", "read on every call", "a group of its own", "caller's order", "k_align_pairs_dirs<carry in LDS>",
                  "k_align_pairs_dirs<carry in global memory>", "Banded and long"):
        assert words in comment, words


def test_design_counts_the_entry_points_and_has_the_section():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(msc_\w+)\s*\(", text))
    assert set(NAMES) <= declared
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"\((\d+) entry points", design)
    assert m and int(m.group(1)) == len(declared), (m and m.group(1), len(declared))
    assert "### 4.6h" in design and all(name in design for name in NAMES)
    section = design[design.index("### 4.6h"):design.index("### 4.7")]
    for words in ("k_align_pairs_dirs", "k_align_trace_count", "k_align_trace_write", "kAlignTraceBytes", "MSC_ALIGN_TRACE_BYTES", "run << 4 | op", "real", "VGPRs", "scratch",
                  "profiles/align_trace.md", "32 767"):
        assert words in section, words
    switches = design[design.index("## 9. Switches"):]
    assert "MSC_ALIGN_TRACE_BYTES" in switches
    assert "traceback" in design[design.index("## 8. What comes next"):design.index("## 9. Switches")]
    assert "msc_align_pairs_trace" in open(os.path.join(ROOT, "README.md")).read()


def test_library_exports_them_and_the_layers_carry_them():
    lib = _capi.load_library()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.PROTOTYPES
    assert _capi.PROTOTYPES[NAMES[0]][1] == _capi.PROTOTYPES["msc_align_pairs"][1] + [C.c_void_p]
    assert len(_capi.PROTOTYPES[NAMES[1]][1]) == 4
    text, offsets, idx = (C.c_uint8 * 2)(65, 0), (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 1)(0)
    out, off, ops = (C.c_int32 * 1)(-7), (C.c_uint64 * 2)(99, 99), (C.c_uint32 * 1)(5)
    assert lib.msc_align_pairs_trace(None, text, offsets, 1, idx, idx, 1, 1, -1, 2, 1, out, out, out, off) == -1          # MSC_ERR_INVALID_ARG
    assert out[0] == -7 and list(off) == [99, 99]
    assert lib.msc_align_pairs_trace_fetch(None, 0, 1, ops) == -1 and ops[0] == 5
    assert lib.msc_abi_version() == 1
    mirror = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"struct\s+Traces\s*:\s*Alignments", mirror) and re.search(r"inline\s+Traces\s+align_pairs_trace\s*\(", mirror)
    assert "msc_align_pairs_trace(" in mirror and "msc_align_pairs_trace_fetch(" in mirror and re.search(r"std::string\s+cigar\s*\(\s*size_t\s+p\s*\)\s*const", mirror)


def test_every_declared_symbol_is_still_exported():
    from tests.test_abi_cpu import test_library_exports_every_declared_symbol
    test_library_exports_every_declared_symbol()


def test_api_call_raises_cleanly_without_a_device():
    out = tuple(np.full(2, -7, dtype=np.int32) for _ in range(3)) + (np.full(3, 99, dtype=np.uint64),)
    with pytest.raises(api.MscError) as e:
        api.align_pairs_trace(None, [b"ACGT", "ACCT"], [0, 1], [1, 1], out=out)
    assert e.value.code == -1 and "Context" in str(e.value) and "msc_align_pairs_trace" in str(e.value)
    assert all((o == -7).all() for o in out[:3]) and (out[3] == 99).all()
    with pytest.raises(ValueError):
        api.align_pairs_trace(None, [b"ACGT"], [0, 0], [0])
    assert api.cigar_string(np.array([120 << 4 | 7, 1 << 4 | 8, 3 << 4 | 1, 2 << 4 | 2], dtype=np.uint32)) == "120=1X3I2D"
    assert api.cigar_string([]) == ""


SNIPPET = r"""
#include "meshclust2_host.hpp"
size_t use(msc::Context& ctx) {
	std::vector<std::string> seqs(2, "ACGT");
	std::vector<uint32_t> first(1, 0), second(1, 1);
	msc::Traces t = msc::align_pairs_trace(ctx, seqs, first, second);
	msc::Traces set = msc::align_pairs_trace(ctx, seqs, first, second, 2, -3, 5, 2);
	const msc::Alignments& base = t;
	return t.cigar(0).size() + set.ops.size() + (size_t)t.op_offsets[1] + (size_t)base.score[0] + (size_t)t.identity[0];
}
int main() {
	msc::Traces t;
	t.op_offsets = {0, 4};
	t.ops = {120u << 4 | 7u, 1u << 4 | 8u, 3u << 4 | 1u, 2u << 4 | 2u};
	return t.cigar(0) == "120=1X3I2D" ? 0 : 1;
}
"""


def test_cpp_host_mirror_carries_the_call(tmp_path):
    src = tmp_path / "align_trace_snippet.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "align_trace_snippet"
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I", host, str(src), "-L", os.path.join(ROOT, "meshclust2_amd"), "-lmeshclust2_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "meshclust2_amd"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert subprocess.run([str(exe)], timeout=60).returncode == 0


def test_fastcar_usage_describes_cigar():
    text = open(os.path.join(ROOT, "meshclust2_amd", "host", "msc_fastcar.cpp")).read()
    usage = text[:text.index("#include")]
    assert "[--align-band W] [--cigar]" in usage
    about = usage[usage.index("// --cigar"):]
    for words in ("with --align", "--align-band", "msc_align_pairs_trace", "DESIGN.md 4.6h", "32 767", "prints *", "reversed", "every output byte is what it was"):
        assert words in about, words
    assert "msc::align_pairs_trace(" in text and text.count("[--align-band W] [--cigar]") == 2
