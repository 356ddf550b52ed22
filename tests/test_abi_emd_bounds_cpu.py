"""msc_set_emd_bounds / msc_last_emd_walk through the public layers, without a device: the header declares them, the built library
exports them, the ctypes table and api.Context carry them, the C++ mirror has the switch, and a NULL context is refused."""
import ctypes
import os
import re

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_both():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+msc_set_emd_bounds\s*\(\s*msc_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", text)
    assert re.search(r"\bint\s+msc_last_emd_walk\s*\(\s*const\s+msc_ctx\s*\*\s*ctx\s*,\s*uint64_t\s*\*\s*listed_pairs\s*,\s*uint64_t\s*\*\s*dense_blocks\s*,\s*uint64_t\s*\*\s*blocks\s*\)\s*;", text)
    lib = _capi.load_library()
    for name in ("msc_set_emd_bounds", "msc_last_emd_walk"):
        assert hasattr(lib, name) and name in _capi.PROTOTYPES
    assert lib.msc_set_emd_bounds(None, 1) == -1          # MSC_ERR_INVALID_ARG: no context
    v = ctypes.c_uint64(7)
    assert lib.msc_last_emd_walk(None, ctypes.byref(v), None, None) == -1 and v.value == 7


def test_context_and_cxx_mirror_have_the_switch():
    assert callable(getattr(api.Context, "set_emd_bounds", None)) and callable(getattr(api.Context, "last_emd_walk", None))
    text = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"void\s+set_emd_bounds\s*\(\s*bool\s+on\s*\)\s*\{\s*check\(msc_set_emd_bounds\(", text)
