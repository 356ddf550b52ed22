import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "ref: checked against the compiled reference (oracle/_ref), replayed from tests/golden/ref_tapes where it is not built")
    expr = config.getoption("markexpr", "") or ""
    if "gpu" in expr and "not gpu" not in expr:
        # One HIP runtime per process: torch ships its own libamdhip64 and reports "No HIP GPUs" when /opt/rocm's copy (which
        # libmeshclust2_hip.so would pull in) is loaded first. The tests that hand device memory to torch (RCCL views) need
        # torch imported before the library, exactly as bench.py does.
        import torch  # noqa: F401


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle_py
    oracle_py.lib()
    return oracle_py


@pytest.hookimpl(hookwrapper=True)
def pytest_runtest_makereport(item, call):
    rep = (yield).get_result()
    if rep.when == "call":
        item.ref_tape_passed = rep.passed


@pytest.fixture
def ref(request):
    """the compiled reference, replayed from tests/golden/ref_tapes/ (tests/ref_tape.py; MSC_REF_TAPE=live / record call the library)"""
    from ref_tape import RefTape
    tape = RefTape(request.node.module.__name__.rsplit(".", 1)[-1], request.node.name)
    yield tape
    tape.close(getattr(request.node, "ref_tape_passed", False))


GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
