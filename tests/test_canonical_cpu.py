"""msc_hist_canonical_batch and the --canonical switches through the public layers, without a device: the numpy helper the GPU tests rely on is held
to the oracle's histograms (strand symmetry, palindromic bins), the header declares the call with the documented signature and states its rules,
the built library exports it, the ctypes table, the api class and the C++ mirror carry it, a call without a context is MSC_ERR_INVALID_ARG, both
drivers name [--canonical] in their usage lines, msc_fastcar refuses it beside --both-strands and the rank driver of msc_cluster refuses it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from canonical_util import canon, one_mers, palindromes, rc_perm, rc_string
from meshclust2_amd import _capi, api
from oracle import oracle_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

SIGNATURE = """int msc_hist_canonical_batch(msc_ctx* ctx, msc_hist_set* dst, const uint32_t* dst_slots,
                             const msc_hist_set* src, const uint32_t* src_slots, uint64_t n);"""


def _hist(s, k, bits):
    oh = oracle_py.hist(s, k, bits)
    try:
        return oh.array().copy()
    finally:
        oracle_py.lib().orc_hist_free(oh)


@pytest.mark.parametrize("k", [3, 4, 9])
def test_the_helper_is_strand_neutral_on_the_oracles_histograms(k):
    rs = np.random.RandomState(100 + k)
    pal = palindromes(k)
    assert (pal.size > 0) == (k % 2 == 0)
    p = rc_perm(k)
    assert np.array_equal(p[p], np.arange(p.size)), "rc is an involution"
    for bits, n in ((16, 400), (32, 1500), (8, 90)):
        s = ACGT[rs.randint(0, 4, n)].tobytes()
        if k % 2 == 0:
            s += (b"ACGT" * 5 if k == 4 else b"")          # palindromic 4-mers, counted several times
        h, hr = _hist(s, k, bits), _hist(rc_string(s), k, bits)
        assert np.array_equal(hr, h[p]), "the histogram of rc(s) is the permuted histogram"
        c, ovf = canon(h, k)
        cr, ovf_r = canon(hr, k)
        assert np.array_equal(c, cr) and ovf == ovf_r
        assert np.array_equal(c, c[p]), "symmetric under rc"
        wide = h.astype(np.int64)
        assert np.array_equal(c[pal].astype(np.int64), np.minimum(2 * wide[pal] - 1, np.iinfo(h.dtype).max))
        assert c.dtype == h.dtype


def test_the_helper_saturates_and_carries():
    h = np.ones(64, dtype=np.uint8)
    h[0], h[63] = 151, 151          # AAA and TTT
    c, ovf = canon(h, 3)
    assert c[0] == c[63] == 255 and ovf and c[1] == 1
    h[0], h[63] = 128, 128          # 255 exactly: no overflow
    c, ovf = canon(h, 3)
    assert c[0] == 255 and not ovf
    w = np.ones(64, dtype=np.uint64)
    w[0], w[63] = 2 ** 63, 2 ** 63          # exact sum 2^64 - 1: fits
    c, ovf = canon(w, 3)
    assert int(c[0]) == 2 ** 64 - 1 and not ovf
    w[0] = 2 ** 63 + 1
    c, ovf = canon(w, 3)
    assert int(c[0]) == 2 ** 64 - 1 and ovf
    z = np.zeros(64, dtype=np.uint16)          # uploaded bins without the pseudocount: clamped at 0
    assert not canon(z, 3)[0].any()
    assert one_mers([5, 6, 7, 8]).tolist() == [12, 12, 12, 12]


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def _header():
    return open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()


def test_header_declares_the_signature():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+msc_hist_canonical_batch\s*\([^;]*\)\s*;", text)
    assert m, "msc_hist_canonical_batch is not declared"
    assert _tokens(m.group(0)) == _tokens(SIGNATURE), m.group(0)
    assert re.search(r"#define\s+MSC_ABI_VERSION\s+1\b", _header())


def test_header_comment_states_the_rules():
    text = _header()
    assert "int msc_hist_canonical_batch" in text
    op = text[:text.index("int msc_hist_canonical_batch")].rsplit("/*", 1)[1]
    for words in ("in-place", "one_mers", "MSC_ERR_OOM", "MSC_ERR_INVALID_ARG", "fastcar/FC_Runner.cpp:426-471", "clutil/Loader.cpp:138-179", "D[b] + D[rc(b)] - 1",
                  "byte-identical", "leaves the old one behind"):
        assert words in op, words


def test_library_exports_it_and_the_layers_carry_it():
    lib = _capi.load_library()
    assert hasattr(lib, "msc_hist_canonical_batch")
    restype, argtypes = _capi.PROTOTYPES["msc_hist_canonical_batch"]
    assert restype is C.c_int and len(argtypes) == 6
    slots = (C.c_uint32 * 1)()
    assert lib.msc_hist_canonical_batch(None, None, slots, None, slots, 1) == -1          # MSC_ERR_INVALID_ARG
    assert callable(getattr(api.HistogramSet, "canonical_batch", None))
    mirror = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"void\s+canonical_batch\s*\(", mirror) and "msc_hist_canonical_batch(" in mirror


def _exe(name):
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    exe = os.path.join(host, name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    return exe


def _run(argv, env=None):
    return subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=env)


@pytest.mark.parametrize("name", ["msc_cluster", "msc_fastcar"])
def test_usage_names_the_flag(name):
    r = _run([_exe(name)])
    assert r.returncode == 1 and b"usage:" in r.stdout and b"[--canonical]" in r.stdout, r.stdout


def test_fastcar_refuses_the_flag_beside_both_strands():
    r = _run([_exe("msc_fastcar"), "db.fa", "--query", "q.fa", "--recover", "w.txt", "--canonical", "--both-strands"])
    assert r.returncode == 1 and b"--canonical" in r.stdout and b"--both-strands" in r.stdout, r.stdout
    r = _run([_exe("msc_fastcar"), "db.fa", "--query", "q.fa", "--recover", "w.txt", "--both-strands", "--top", "3"])          # the older refusal stays
    assert r.returncode == 1 and b"--both-strands" in r.stdout and b"--top" in r.stdout, r.stdout


def test_the_rank_driver_refuses_the_flag():
    env = dict(os.environ, MSC_FORCE_SHARDED="1")
    env.pop("WORLD_SIZE", None)
    r = _run([_exe("msc_cluster"), "x.fa", "--canonical"], env=env)
    assert r.returncode == 1 and b"--canonical" in r.stdout, r.stdout
