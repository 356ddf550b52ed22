"""msc_set_fold_screen / msc_last_fold_screen / msc_fold_bin through the public layers, without a device: the header declares them, the
built library exports them, the ctypes table and api.Context carry them, the C++ mirror has the switch, a NULL context is refused -- and
the fold map itself, against its numpy form for every bin at k = 5 .. 9 and the three folds."""
import ctypes
import os
import re

import numpy as np

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+msc_set_fold_screen\s*\(\s*msc_ctx\s*\*\s*ctx\s*,\s*int\s+fold\s*\)\s*;", text)
    assert re.search(r"\bint\s+msc_last_fold_screen\s*\(\s*const\s+msc_ctx\s*\*\s*ctx\s*,\s*uint64_t\s*\*\s*fold\s*,\s*uint64_t\s*\*\s*folded_blocks\s*,\s*uint64_t\s*\*\s*fell_back\s*\)\s*;", text)
    assert re.search(r"\buint64_t\s+msc_fold_bin\s*\(\s*uint64_t\s+bin\s*,\s*uint64_t\s+nbins\s*,\s*uint32_t\s+fold\s*\)\s*;", text)
    lib = _capi.load_library()
    for name in ("msc_set_fold_screen", "msc_last_fold_screen", "msc_fold_bin"):
        assert hasattr(lib, name) and name in _capi.PROTOTYPES
    assert lib.msc_set_fold_screen(None, 16) == -1          # MSC_ERR_INVALID_ARG: no context
    v = ctypes.c_uint64(7)
    assert lib.msc_last_fold_screen(None, ctypes.byref(v), None, None) == -1 and v.value == 7


def test_context_and_cxx_mirror_have_the_switch():
    for name in ("set_fold_screen", "last_fold_screen"):
        assert callable(getattr(api.Context, name, None))
    assert callable(api.fold_bin)
    text = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"void\s+set_fold_screen\s*\(\s*int\s+fold\s*\)\s*\{\s*check\(msc_set_fold_screen\(", text)


def test_fold_bin_is_the_bin_modulo_the_folded_size():
    lib = _capi.load_library()
    for k in range(5, 10):
        nbins = 4 ** k
        bins = np.arange(nbins, dtype=np.uint64)
        for fold in (8, 16, 32):
            got = np.fromiter((lib.msc_fold_bin(int(b), nbins, fold) for b in bins), dtype=np.uint64, count=nbins)
            assert np.array_equal(got, bins % np.uint64(nbins // fold)), (k, fold)
            assert got.max() == nbins // fold - 1
    assert api.fold_bin(12345, 4 ** 9, 0) == 12345 and api.fold_bin(12345, 4 ** 9, 1) == 12345
    assert api.fold_bin(4 ** 9 - 1, 4 ** 9, 16) == 4 ** 9 // 16 - 1
