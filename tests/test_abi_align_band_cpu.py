"""msc_align_pairs_banded and msc_align_pairs_auto through the public layers, without a device: the header declares both after
msc_align_pairs with the documented signatures and states their rules, the built library exports them, the ctypes table, api.py and the C++
host mirror carry them, a call without a context is refused cleanly and leaves its outputs alone, DESIGN.md counts them, msc_fastcar names
[--align-band W] and refuses it without --align before it opens a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BANDED = """int msc_align_pairs_banded(msc_ctx* ctx,
                           const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                           const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                           int match, int mismatch, int gap_open, int gap_continue, uint32_t band,
                           int32_t* score, int32_t* length, int32_t* matches, uint8_t* certified);"""
AUTO = """int msc_align_pairs_auto(msc_ctx* ctx,
                         const uint8_t* seqs, const uint64_t* offsets, uint64_t n_seqs,
                         const uint32_t* first, const uint32_t* second, uint64_t n_pairs,
                         int match, int mismatch, int gap_open, int gap_continue, uint32_t first_band,
                         int32_t* score, int32_t* length, int32_t* matches, uint32_t* band_used);"""


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def _header():
    return open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()


def test_header_declares_both_signatures_after_msc_align_pairs():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    at = []
    for name, signature in (("msc_align_pairs", None), ("msc_align_pairs_banded", BANDED), ("msc_align_pairs_auto", AUTO)):
        m = re.search(r"\bint\s+%s\s*\([^;]*\)\s*;" % name, text)
        assert m, name + " is not declared"
        assert signature is None or _tokens(m.group(0)) == _tokens(signature), m.group(0)
        at.append(m.start())
    assert at == sorted(at)
    assert re.search(r"#define\s+MSC_ABI_VERSION\s+1\b", _header())          # the change is additive


def test_header_comment_states_the_rules():
    text = _header()
    comment = text[:text.index("int msc_align_pairs_banded")].rsplit("/* ---", 1)[1]
    assert "int msc_align_pairs(" not in comment          # a block of their own
    for words in ("DESIGN.md 4.6f", "certified[p] = 1", "PROVEN", "bit for bit", "-2^30", "gap_open >= 0, gap_continue >= 0 and max(match, mismatch) + 2 * gap_continue >= 0",
                  "0xffffffff", "first_band (0: the library's default", "may be NULL", "1 .. 32 767", "at most 100", "MSC_ERR_INVALID_ARG", "n_pairs == 0 is MSC_OK", "untouched",
                  "k_align_band<", "k_align_pairs", "caller's order", "Worth it from", "uploaded once"):
        assert words in comment, words


def test_design_counts_the_entry_points_and_has_the_section():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(msc_\w+)\s*\(", text))
    assert {"msc_align_pairs_banded", "msc_align_pairs_auto"} <= declared
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"\((\d+) entry points", design)
    assert m and int(m.group(1)) == len(declared), (m and m.group(1), len(declared))
    assert "4.6f" in design and "msc_align_pairs_banded" in design and "msc_align_pairs_auto" in design


def test_library_exports_them_and_the_layers_carry_them():
    lib = _capi.load_library()
    text, offsets, idx = (C.c_uint8 * 2)(65, 0), (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 1)(0)
    for name in ("msc_align_pairs_banded", "msc_align_pairs_auto"):
        assert hasattr(lib, name)
        restype, argtypes = _capi.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == 16
        assert argtypes[3] is C.c_uint64 and argtypes[6] is C.c_uint64 and all(argtypes[i] is C.c_int for i in (7, 8, 9, 10)) and argtypes[11] is C.c_uint32
        out, last = (C.c_int32 * 1)(-7), (C.c_uint32 * 1)(77)
        assert getattr(lib, name)(None, text, offsets, 1, idx, idx, 1, 1, -1, 2, 1, 8, out, out, out, last) == -1          # MSC_ERR_INVALID_ARG
        assert out[0] == -7 and last[0] == 77
    assert lib.msc_abi_version() == 1
    mirror = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"inline\s+BandedAlignments\s+align_pairs_banded\s*\(", mirror) and "msc_align_pairs_banded(" in mirror
    assert re.search(r"inline\s+BandedAlignments\s+align_pairs_auto\s*\(", mirror) and "msc_align_pairs_auto(" in mirror
    assert re.search(r"struct\s+Alignments\s*\{\s*std::vector<int32_t> score, length, matches;\s*std::vector<double> identity;\s*\};", mirror)          # as it was


def test_every_declared_symbol_is_still_exported():
    from tests.test_abi_cpu import test_library_exports_every_declared_symbol
    test_library_exports_every_declared_symbol()


def test_api_calls_raise_cleanly_without_a_device():
    for call, last, kw in ((api.align_pairs_banded, np.uint8, dict(band=4)), (api.align_pairs_auto, np.uint32, dict(first_band=4))):
        out = tuple(np.full(2, -7, dtype=np.int32) for _ in range(3)) + (np.full(2, 9, dtype=last),)
        with pytest.raises(api.MscError) as e:
            call(None, [b"ACGT", "ACCT"], [0, 1], [1, 1], out=out, **kw)
        assert e.value.code == -1 and "Context" in str(e.value)
        assert all((o == -7).all() for o in out[:3]) and (out[3] == 9).all()
        with pytest.raises(ValueError):
            call(None, [b"ACGT"], [0, 0], [0], **kw)
        with pytest.raises(ValueError):
            call(None, [b"ACGT"], [0], [0], **{k: -1 for k in kw})
        with pytest.raises(ValueError):          # the fourth output has the call's own type
            call(None, [b"ACGT"], [0], [0], out=tuple(np.zeros(1, dtype=np.int32) for _ in range(4)), **kw)


SNIPPET = r"""
#include "meshclust2_host.hpp"
double use(msc::Context& ctx) {
	std::vector<std::string> seqs(2, "ACGT");
	std::vector<uint32_t> first(1, 0), second(1, 1);
	msc::BandedAlignments a = msc::align_pairs_banded(ctx, seqs, first, second, 16);
	msc::BandedAlignments b = msc::align_pairs_banded(ctx, seqs, first, second, 16, 2, -3, 5, 2);
	msc::BandedAlignments c = msc::align_pairs_auto(ctx, seqs, first, second);
	msc::BandedAlignments d = msc::align_pairs_auto(ctx, seqs, first, second, 64, 2, -3, 5, 2);
	msc::Alignments full = msc::align_pairs(ctx, seqs, first, second);
	const bool filled = d.band_used[0] == msc::BandedAlignments::no_band;
	return a.identity[0] + b.score[0] + b.certified[0] + c.length[0] + c.band_used[0] + d.matches[0] + full.identity[0] + (filled ? 1 : 0);
}
int main() { return msc::BandedAlignments::no_band == 0xffffffffu ? 0 : 1; }
"""


def test_cpp_host_mirror_carries_the_calls(tmp_path):
    src = tmp_path / "align_band_snippet.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "align_band_snippet"
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


def test_fastcar_names_the_flag_and_refuses_it_without_align():
    r = subprocess.run([_fastcar()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 1 and b"usage:" in r.stdout and b"[--align]" in r.stdout and b"[--align-band W]" in r.stdout, r.stdout
    # the files do not exist and there may be no device: the refusal comes before either is looked at
    r = subprocess.run([_fastcar(), "db.fa", "--query", "q.fa", "--recover", "w.txt", "--align-band", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 1 and b"--align-band" in r.stdout and b"--align" in r.stdout and b"msc error" not in r.stdout, r.stdout
