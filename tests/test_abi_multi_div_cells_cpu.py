"""msc_set_multi_div_cells through the public layers, without a device: the header declares it, the built library exports it, the ctypes
table and api.Context carry it, the C++ mirror has the method, and a NULL context is refused."""
import os
import re

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_switch():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+msc_set_multi_div_cells\s*\(\s*msc_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", text)
    lib = _capi.load_library()
    assert hasattr(lib, "msc_set_multi_div_cells")
    assert "msc_set_multi_div_cells" in _capi.PROTOTYPES
    assert lib.msc_set_multi_div_cells(None, 1) == -1          # MSC_ERR_INVALID_ARG: no context
    assert lib.msc_set_multi_div_cells(None, 0) == -1


def test_context_has_the_method():
    assert callable(getattr(api.Context, "set_multi_div_cells", None))
    assert callable(getattr(api.Context, "set_pairs_div_cells", None))          # the two switches are separate


def test_cxx_mirror_has_the_method():
    text = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"void\s+set_multi_div_cells\s*\(\s*bool\s+on\s*\)\s*\{\s*check\(msc_set_multi_div_cells\(", text)
