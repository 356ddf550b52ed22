"""The histogram builders (hist_build.hip, sparse.hip), route by route: every setting of MSC_NO_LDS_BUILD, MSC_NO_SORT_DENSE_BUILD and
MSC_NO_SORT_BUILD that moves a batch to another builder runs build_route_check.py in a child process (the library reads the switches
once per process), which holds every slot to a reference computed outside the library and asserts the builder
msc_hist_set_build_info names. A last test compares what the variants dumped."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("MSC_NO_LDS_BUILD", "MSC_NO_SORT_DENSE_BUILD", "MSC_NO_SORT_BUILD", "MSC_HOST_THREADS", "MSC_TRACE_CALLS")
# (name, switches, time limit in s). The first variant also computes the reference, which the others read back.
VARIANTS = [("default", "", 120),
            ("no_lds", "MSC_NO_LDS_BUILD", 60),
            ("no_sort_dense", "MSC_NO_SORT_DENSE_BUILD", 60),
            ("no_lds_no_sort_dense", "MSC_NO_LDS_BUILD MSC_NO_SORT_DENSE_BUILD", 60),
            ("no_sort_sparse", "MSC_NO_SORT_BUILD", 60)]
DENSE_A = [(1, 16), (2, 32), (3, 8), (4, 16), (5, 16), (6, 64), (7, 8), (7, 32), (7, 64), (8, 8), (8, 16), (9, 32), (10, 8)]
SPARSE_A = [(8, 8), (9, 32), (11, 8), (13, 64)]


def route_a(k, bits, sparse, switches):
    """the builder of a batch of short sequences. Dense: k <= 7 is k_build_lds except (7, 64), whose 32 tiles are beyond it; without the
    LDS builder (7, 32) has the 16 tiles k_build_sort needs and every smaller histogram goes to k_count; without the dense sort builder
    whatever it took goes to k_count. Sparse: k_sparse_build_sort, or dense scratch slots (short sequences: built by k_build_sort) + compaction."""
    if sparse:
        return "k_build_sort+k_sparse_write" if "MSC_NO_SORT_BUILD" in switches else "k_sparse_build_sort"
    if k >= 8 or (k, bits) == (7, 64):
        name = "k_build_sort"
    elif "MSC_NO_LDS_BUILD" not in switches:
        name = "k_build_lds"
    else:
        name = "k_build_sort" if (k, bits) == (7, 32) else "k_count"
    return "k_count" if name == "k_build_sort" and "MSC_NO_SORT_DENSE_BUILD" in switches else name


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    return tmp_path_factory.mktemp("build_routes")


_TROUBLE = []          # variants whose child faulted, aborted or hung: nothing more is started on the GPU after one


def run_variant(dumps, name, switches, timeout):
    if _TROUBLE:
        pytest.fail("not started: variant %s ended with %s" % _TROUBLE[0])
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    for sw in switches.split():
        env[sw] = "1"
    try:
        out = subprocess.run([sys.executable, os.path.join(HERE, "build_route_check.py"), str(dumps / name), str(dumps / "oracle")], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired:
        _TROUBLE.append((name, "no result within %d s" % timeout))
        raise
    if out.returncode not in (0, 1):          # (1: a failed check; anything else -- an abort, a signal -- may have left the GPU in trouble)
        _TROUBLE.append((name, "exit status %d" % out.returncode))
    assert b"BUILD_ROUTE_OK" in out.stdout, out.stdout.decode(errors="replace")[-3000:]


@pytest.mark.parametrize("name,switches,timeout", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_build_route_variant(dumps, name, switches, timeout):
    """one setting of the builder switches against the reference: the route table (k = 1 .. 10 dense, k = 8 .. 13 sparse), 0 .. 32768 and
    32769 k-mers per sequence, u8 bins at 254 / 255 / 256 and 128 saturated bins at once, u16 bins at 65535 with and without the overflow
    flag, segments at every offset of the packed stream and on its last base, records without k-mers, ungrouped segment lists, the
    stream in device memory, rebuilt slots and the set's bounds, upload(), lists of more than 32768 k-mers at k = 11 and k = 13"""
    run_variant(dumps, name, switches, timeout)


def test_build_route_dumps_agree(dumps):
    """every array of every variant -- scalar records, tile prefixes, raw slots, packed sparse slots, bounds -- is bit-identical to the
    default's. One field is left out of that: the stddev word of the records (cleared in the dumps). Each builder evaluates that FP64
    expression in a kernel of its own, and whether two kernels round it alike is a matter of the compiler's contraction of multiply-adds
    (off in today's build), not of the builders; <case>.std.npy holds it per slot beside the extended-precision value and the derived
    tolerance (build_route_check.py), which every variant must meet. The builder names of the
    route table are the ones the switches must give, so each variant differs from the default exactly there."""
    failed = []
    for v in VARIANTS:
        d = dumps / v[0]
        if (d / "DONE").exists():
            continue
        if (d / "STARTED").exists():          # ran and failed (its own test says why): never run again
            failed.append(v[0])
        else:                                  # never ran (this test run alone)
            run_variant(dumps, *v)
    assert not failed, "variants that ran and left no result: %s" % failed
    names = sorted(p.name for p in (dumps / "default").iterdir() if p.suffix == ".npy")
    for case in "ABCDEF":
        assert sum(n.startswith(case + "_") for n in names) >= 4, (case, names)
    for v in VARIANTS:
        assert sorted(p.name for p in (dumps / v[0]).iterdir() if p.suffix == ".npy") == names, v[0]
    for f in names:
        base = np.load(dumps / "default" / f)
        for v in VARIANTS:
            got = np.load(dumps / v[0] / f)
            assert got.shape == base.shape and got.dtype == base.dtype, (f, v[0])
            if f.endswith(".std.npy"):          # columns: the builder's stddev, the extended-precision value, the absolute tolerance
                assert np.array_equal(got[:, 1:], base[:, 1:]), (f, v[0])
                assert (np.abs(got[:, 0] - got[:, 1]) <= got[:, 2]).all(), (f, v[0], got)
            else:
                assert np.array_equal(got, base), (f, v[0])
    routes = {v[0]: json.load(open(dumps / v[0] / "routes.json")) for v in VARIANTS}
    table = [("A_dense_k%d_u%d" % kb, kb, False) for kb in DENSE_A] + [("A_sparse_k%d_u%d" % kb, kb, True) for kb in SPARSE_A]
    for v in VARIANTS:
        assert sorted(routes[v[0]]) == sorted(routes["default"]), v[0]
        for key, (k, bits), sparse in table:
            assert routes[v[0]][key] == route_a(k, bits, sparse, v[1].split()), (v[0], key, routes[v[0]][key])
        moved = {key for key, _, _ in table if routes[v[0]][key] != routes["default"][key]}
        assert moved == {key for key, (k, bits), sparse in table if route_a(k, bits, sparse, v[1].split()) != route_a(k, bits, sparse, [])}, (v[0], moved)
        assert (v[0] == "default") == (not moved), v[0]
    assert [routes["default"]["A_dense_k%d_u%d" % kb] for kb in DENSE_A if kb[0] <= 7].count("k_build_sort") == 1      # (7, 64) alone
    lds_off = routes["no_lds"]
    assert lds_off["A_dense_k7_u32"] == "k_build_sort" and {lds_off["A_dense_k%d_u%d" % kb] for kb in ((1, 16), (2, 32), (3, 8))} == {"k_count"}
