"""msc_set_sparse_matrix_pass through the public layers, without a device: the header declares it, the built library exports it, the
ctypes table and api.Context carry it, and msc_fastcar names --sparse-matrix in its usage line."""
import os
import re
import subprocess

from meshclust2_amd import _capi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_switch():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+msc_set_sparse_matrix_pass\s*\(\s*msc_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", text)
    lib = _capi.load_library()
    assert hasattr(lib, "msc_set_sparse_matrix_pass")
    assert "msc_set_sparse_matrix_pass" in _capi.PROTOTYPES
    assert lib.msc_set_sparse_matrix_pass(None, 1) == -1          # MSC_ERR_INVALID_ARG: no context


def test_context_has_the_method():
    assert callable(getattr(api.Context, "set_sparse_matrix_pass", None))


def test_fastcar_usage_names_the_flag():
    host = os.path.join(ROOT, "meshclust2_amd", "host")
    exe = os.path.join(host, "msc_fastcar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 1 and b"usage:" in r.stdout and b"[--sparse-matrix]" in r.stdout, r.stdout
