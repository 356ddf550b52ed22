"""msc_align_pairs_long, msc_align_pairs_long_banded and msc_align_pairs_long_auto through the public layers, without a device: the header
declares them after msc_align_pairs_auto with the signatures of their namesakes and states their rules, the built library exports them, the
ctypes table, api.py and the C++ host mirror carry them, a call without a context is refused cleanly and leaves its outputs alone, DESIGN.md
counts them and lists the two switches, msc_fastcar's usage comment no longer states the old limit for --align."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msc_align_pairs_long", "msc_align_pairs_long_banded", "msc_align_pairs_long_auto")


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def _header():
    return open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()


def _declaration(text, name):
    m = re.search(r"\bint\s+%s\s*\([^;]*\)\s*;" % name, text)
    assert m, name + " is not declared"
    return m


def test_header_declares_the_signatures_of_the_namesakes():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    at = [_declaration(text, "msc_align_pairs_auto").start()]
    for name in NAMES:
        short, long_one = _declaration(text, name.replace("_long", "")), _declaration(text, name)
        assert _tokens(long_one.group(0)) == [name if t == name.replace("_long", "") else t for t in _tokens(short.group(0))], long_one.group(0)
        at.append(long_one.start())
    assert at == sorted(at)
    assert re.search(r"#define\s+MSC_ABI_VERSION\s+1\b", _header())          # the change is additive


def test_header_comment_states_the_rules():
    text = _header()
    comment = text[:text.index("int msc_align_pairs_long(")].rsplit("/* ---", 1)[1]
    assert "int msc_align_pairs_auto(" not in comment          # a block of their own
    for words in ("DESIGN.md 4.6g", "1 .. 1 048 575", "kAlignLongMaxLen", "at most 100", "MSC_ERR_INVALID_ARG", "untouched", "n_pairs == 0 is MSC_OK", "keep their limit of 32 767",
                  "bit for bit", "-2^30", "MSC_ALIGN_LONG_ALL=1", "MSC_ALIGN_TILE_ROWS", "read on every call", "caller's order", "k_align_tiles<", "first_band (0: the library's default",
                  "may be NULL", "0xffffffff", "`first` is sequence 1"):
        assert words in comment, words


def test_design_counts_the_entry_points_and_has_the_section():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(msc_\w+)\s*\(", text))
    assert set(NAMES) <= declared
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"\((\d+) entry points", design)
    assert m and int(m.group(1)) == len(declared), (m and m.group(1), len(declared))
    assert "4.6g" in design and all(name in design for name in NAMES)
    for words in ("MSC_ALIGN_LONG_ALL", "MSC_ALIGN_TILE_ROWS", "1 048 575", "k_align_tiles"):
        assert words in design, words


def test_library_exports_them_and_the_layers_carry_them():
    lib = _capi.load_library()
    text, offsets, idx = (C.c_uint8 * 2)(65, 0), (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 1)(0)
    for name in NAMES:
        assert hasattr(lib, name)
        restype, argtypes = _capi.PROTOTYPES[name]
        assert (restype, argtypes) == _capi.PROTOTYPES[name.replace("_long", "")]
        out, last = (C.c_int32 * 1)(-7), (C.c_uint32 * 1)(77)
        args = (None, text, offsets, 1, idx, idx, 1, 1, -1, 2, 1) + ((8,) if len(argtypes) == 16 else ()) + (out, out, out) + ((last,) if len(argtypes) == 16 else ())
        assert getattr(lib, name)(*args) == -1          # MSC_ERR_INVALID_ARG
        assert out[0] == -7 and last[0] == 77
    assert lib.msc_abi_version() == 1
    mirror = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"inline\s+Alignments\s+align_pairs_long\s*\(", mirror) and "msc_align_pairs_long(" in mirror
    assert re.search(r"inline\s+BandedAlignments\s+align_pairs_long_banded\s*\(", mirror) and "msc_align_pairs_long_banded(" in mirror
    assert re.search(r"inline\s+BandedAlignments\s+align_pairs_long_auto\s*\(", mirror) and "msc_align_pairs_long_auto(" in mirror


def test_every_declared_symbol_is_still_exported():
    from tests.test_abi_cpu import test_library_exports_every_declared_symbol
    test_library_exports_every_declared_symbol()


def test_api_calls_raise_cleanly_without_a_device():
    for call, last, kw in ((api.align_pairs_long, None, {}), (api.align_pairs_long_banded, np.uint8, dict(band=4)), (api.align_pairs_long_auto, np.uint32, dict(first_band=4))):
        out = tuple(np.full(2, -7, dtype=np.int32) for _ in range(3)) + ((np.full(2, 9, dtype=last),) if last else ())
        with pytest.raises(api.MscError) as e:
            call(None, [b"ACGT", "ACCT"], [0, 1], [1, 1], out=out, **kw)
        assert e.value.code == -1 and "Context" in str(e.value) and call.__name__.replace("align", "msc_align") in str(e.value)
        assert all((o == -7).all() for o in out[:3]) and all((o == 9).all() for o in out[3:])
        with pytest.raises(ValueError):
            call(None, [b"ACGT"], [0, 0], [0], **kw)


SNIPPET = r"""
#include "meshclust2_host.hpp"
double use(msc::Context& ctx) {
	std::vector<std::string> seqs(2, "ACGT");
	std::vector<uint32_t> first(1, 0), second(1, 1);
	msc::Alignments full = msc::align_pairs_long(ctx, seqs, first, second);
	msc::Alignments set = msc::align_pairs_long(ctx, seqs, first, second, 2, -3, 5, 2);
	msc::BandedAlignments a = msc::align_pairs_long_banded(ctx, seqs, first, second, 16);
	msc::BandedAlignments b = msc::align_pairs_long_banded(ctx, seqs, first, second, 16, 2, -3, 5, 2);
	msc::BandedAlignments c = msc::align_pairs_long_auto(ctx, seqs, first, second);
	msc::BandedAlignments d = msc::align_pairs_long_auto(ctx, seqs, first, second, 64, 2, -3, 5, 2);
	return full.identity[0] + set.score[0] + a.identity[0] + b.certified[0] + c.band_used[0] + d.matches[0];
}
int main() { return 0; }
"""


def test_cpp_host_mirror_carries_the_calls(tmp_path):
    src = tmp_path / "align_long_snippet.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "align_long_snippet"
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I", host, str(src), "-L", os.path.join(ROOT, "meshclust2_amd"), "-lmeshclust2_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "meshclust2_amd"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert subprocess.run([str(exe)], timeout=60).returncode == 0


def test_fastcar_no_longer_states_the_old_limit_for_align():
    text = open(os.path.join(ROOT, "meshclust2_amd", "host", "msc_fastcar.cpp")).read()
    usage = text[:text.index("#include")]
    about = usage[usage.index("// --align:"):]
    assert "(1 .. 32 767 bytes each)" not in about and "1 .. 1 048 575 bytes each" in about
    assert "msc_align_pairs_long" in about and "msc_align_pairs_long_auto" in about
    assert "msc::align_pairs_long(" in text and "msc::align_pairs_long_auto(" in text
