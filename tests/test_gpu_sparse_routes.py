"""The merge kernels of sparse sets (sparse.hip), route by route: every MSC_SPARSE_* switch that selects one of them runs
sparse_route_check.py in a child process (the library reads the switches once per process), which holds each result to the CPU
oracle and asserts the kernel msc_last_kernel_info names. A last test compares the raw statistics the variants dumped."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import FEATS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("MSC_SPARSE_NO_WL", "MSC_SPARSE_MP_NO_PARTS", "MSC_SPARSE_MP_CHUNK", "MSC_SPARSE_MP_NO_PAIRS", "MSC_SPARSE_NO_MP", "MSC_SPARSE_LDS",
            "MSC_SPARSE_NO_MULTI", "MSC_SPARSE_MEAN_NO_GROUPS", "MSC_SPARSE_MEAN_GROUPS_MIN_K", "MSC_SPARSE_MP_DMA", "MSC_TEST_EXPECT_KERNEL")
# (name, switches, the kernel that must score the chunk-end sweep's long lists (None: the checker's rule alone), time limit in s).
# The first variant also computes the oracle's values, which the others read back.
VARIANTS = [("default", "", "k_pair_sparse_mp", 240),
            ("no_wl", "MSC_SPARSE_NO_WL", "k_pair_sparse_mp", 60),
            ("no_parts", "MSC_SPARSE_MP_NO_PARTS", "k_pair_sparse_mp", 60),
            ("chunk512", "MSC_SPARSE_MP_CHUNK=512", "k_pair_sparse_mp", 60),
            ("chunk575", "MSC_SPARSE_MP_CHUNK=575", "k_pair_sparse_mp", 60),
            ("no_pairs", "MSC_SPARSE_MP_NO_PAIRS", "k_pair_sparse_mp", 60),
            ("no_mp", "MSC_SPARSE_NO_MP", "k_pair_sparse", 60),
            ("no_multi", "MSC_SPARSE_NO_MULTI", "k_pair_sparse_mp", 60),
            ("lds", "MSC_SPARSE_LDS", None, 60),
            ("mean_groups5", "MSC_SPARSE_MEAN_GROUPS_MIN_K=5", "k_pair_sparse_mp", 60),
            ("mean_groups16", "MSC_SPARSE_MEAN_GROUPS_MIN_K=16", "k_pair_sparse_mp", 60),
            ("mean_no_groups", "MSC_SPARSE_MEAN_NO_GROUPS", "k_pair_sparse_mp", 60)]
# variants whose divergence sums must equal the default's bit for bit: granule records added in granule order, whatever the window,
# `parts`, the whole-list rule, the staging or the Q x M route. The default chunk is 575 up to k = 11 and 512 from k = 12 on, so the
# variant that forces the default's own chunk belongs here too (chunk575 for the k <= 11 dumps, chunk512 for the k12_ ones). A chunk
# of another size, the lane-per-sub-range and the LDS kernels add the same terms in another order: held to the extended-precision
# value (by the checker).
SAME_DIV_BITS = {"default", "no_wl", "no_parts", "no_pairs", "no_multi", "mean_groups5", "mean_groups16", "mean_no_groups"}
DIV_COLS = [i for i, (n, _) in enumerate(FEATS) if n in ("jefferey_divergence", "jensen_shannon")]
INT_COLS = [i for i in range(len(FEATS)) if i not in DIV_COLS]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    return tmp_path_factory.mktemp("sparse_routes")


_TROUBLE = []          # variants whose child faulted, aborted or hung: nothing more is started on the GPU after one


def run_variant(dumps, name, switches, kernel, timeout):
    if _TROUBLE:
        pytest.fail("not started: variant %s ended with %s" % _TROUBLE[0])
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    for sw in switches.split():
        key, _, val = sw.partition("=")
        env[key] = val or "1"
    if kernel:
        env["MSC_TEST_EXPECT_KERNEL"] = kernel
    try:
        out = subprocess.run([sys.executable, os.path.join(HERE, "sparse_route_check.py"), str(dumps / name), str(dumps / "oracle")], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired:
        _TROUBLE.append((name, "no result within %d s" % timeout))
        raise
    if out.returncode not in (0, 1):          # (1: a failed check; anything else -- an abort, a signal -- may have left the GPU in trouble)
        _TROUBLE.append((name, "exit status %d" % out.returncode))
    assert b"SPARSE_ROUTE_OK" in out.stdout, out.stdout.decode(errors="replace")[-3000:]


@pytest.mark.parametrize("name,switches,kernel,timeout", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_sparse_route_variant(dumps, name, switches, kernel, timeout):
    """one route of the sparse merge kernels against the oracle: chunk ends on ties (512 / 575, at k = 11 and k = 12), empty and
    one-entry lists, 1 against 79 000 entries, windows of 1 .. 7000 (`parts` 16, 8, 4, 2 and 1 of either form), the whole-list fit
    boundary, counts at 255 / 8191 / 8192 / 46340 / 65535 (u32) / 65536 (u64), get_close / filter / merge / merge_all / merge_some /
    update_centres / the mean (grouped and full sweeps), Q x M == 1 x M per query (queries that all fit the whole-list kernel, some, none)"""
    run_variant(dumps, name, switches, kernel, timeout)


def test_sparse_route_dumps_agree(dumps):
    """the integer statistics of every variant are bit-identical, and so are the distances to every rounded mean (mean_*: the grouped
    and the full sweep write one list); the divergence sums too wherever the kernel keeps its granule order.
    Every chunk and mean variant takes another route than the default somewhere (routes.json: the library's rules per case)."""
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
    assert len(names) >= 20, names
    assert sum(f.startswith("mean_") for f in names) >= 20, names
    for f in names:
        base = np.load(dumps / "default" / f)
        same = SAME_DIV_BITS | ({"chunk512"} if f.startswith("k12_") else {"chunk575"})
        for v in VARIANTS[1:]:
            got = np.load(dumps / v[0] / f)
            assert got.shape == base.shape, (f, v[0])
            if f.startswith("mean_"):          # distances to a rounded mean: one list whatever sweep wrote the mean, whatever kernel took |p - r|
                assert np.array_equal(got, base), (f, v[0])
                continue
            if f.startswith("parts_div"):
                cols, int_cols = list(range(base.shape[1])), []
            elif f.startswith("parts_int"):
                cols, int_cols = [], list(range(base.shape[1]))
            else:
                cols, int_cols = DIV_COLS, INT_COLS
            assert np.array_equal(got[:, int_cols], base[:, int_cols], equal_nan=True), (f, v[0])
            if v[0] in same:
                assert np.array_equal(got[:, cols], base[:, cols], equal_nan=True), (f, v[0])
            else:
                assert np.allclose(got[:, cols], base[:, cols], rtol=2e-10, atol=1e-18, equal_nan=True), (f, v[0])
    routes = {v[0]: json.load(open(dumps / v[0] / "routes.json")) for v in VARIANTS}
    for name in ("chunk512", "chunk575", "mean_groups5", "mean_groups16", "mean_no_groups"):
        assert routes[name] != routes["default"], (name, routes[name])
    assert routes["default"]["chunk_ends_chunk"] == 575 and routes["default"]["k12_chunk_ends_chunk"] == 512, routes["default"]
