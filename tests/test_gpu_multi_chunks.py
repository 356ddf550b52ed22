"""msc_score_multi with a block's candidates in several chunks, route by route (tests/multi_chunk_check.py holds the cases and the
comparisons). A block's candidates are cut into equal chunks whenever one launch's scratch would pass a cap -- the product array of the matrix
cores (2 GiB), the group records of sim_mm / rre_k_r (1 GiB, reached with no switch set from 32 769 candidates at 128 queries), the partial
records of the digest, ring and raw-tile kernels (4 GiB) -- and per chunk the drivers re-derive the offset into the slot list, into bins,
scalars and headers, the stride of the divergence records, the group records' query part, the list's capacity and its words, the flag
buffers and the column the results go home to. Every case here runs a call in two or three chunks a block and holds each of its pairs to
the same call over the distinct slots in ONE chunk (gathered by the slot list), which is itself held to the CPU oracle on three query rows x
200 candidates. The number of chunks is asserted in every case (msc_last_kernel_launches against the caps restated in the helper).

The library reads its route switches once per process: one child process per set of switches, one after another."""
import os
import subprocess
import sys

import pytest

from multi_chunk_check import MODE_ENV

pytestmark = pytest.mark.gpu


def _child(mode, timeout):
    tests = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSC_")}
    env.update(MODE_ENV[mode])
    r = subprocess.run([sys.executable, os.path.join(tests, "multi_chunk_check.py"), mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = r.stdout.decode(errors="replace")
    print(out)
    assert r.returncode == 0 and ("MULTI_CHUNK_OK %s" % mode) in out, out[-4000:]


def test_matrix_cores_over_a_slot_list():
    """MSC_GEMM_SLICES=64, 130 queries x 70 000 slots of the 800: the block of 128 in 2 chunks of 35 000, the block of 2 in one.
    The scored tail (sums, nine raw statistics, flags, counts; both argument orders) bit for bit; flags only = the FP64 flags with the list
    path in every chunk, no fold and no tail group for the block in two chunks, and the same flags with every chunk dense under
    msc_set_emd_bounds(0); one chunk of two overflowing its list, in either order of the halves; 8-bit bins under a model without the
    distance. msc_last_emd_walk counts a block once per chunk: asserted as 3 of the 130-query call, 2 of the block of 128.
    The block of 2 runs in one chunk and folds (16-to-1); every related pair of its two queries is then listed, 2.5 % of a uniform draw
    against the list's 1.56 %, so it falls back and runs again with the true product: msc_last_fold_screen says (16, 1, 1) and the call
    takes 3 + 1 launches -- asserted as 3 + fell_back. The call of the first 128 queries alone: 2 launches, no folded block.
    As printed on an MI355X: listed 85 288 of 9 100 000 pairs = 0.94 % in either order, dense 0 of 3 chunks (capacity 1.56 % a chunk); the
    overflow case: dense 1 of 2 chunks whichever half comes first, listed 0 in the other chunk, 50.7 % of the same-family pairs close.
    Child process 2.9 s (scored tail in both orders 2.0 s, the rest 0.4 s)."""
    _child("matrix", 600)


def test_matrix_cores_over_contiguous_candidates():
    """cand_slots = None over an 8-bit set of 70 000 slots (18 GB; slot s holds sequence s mod 2 000): the chunk's offset reaches the bins,
    the scalars, the headers and kb_first. Scored tail in both orders and flags only, against the call over the first 2 000 slots, tiled.
    As printed on an MI355X: listed 11 830 of 9 100 000 pairs = 0.13 % in either order, dense 0 of 3 chunks; the block of 2 folded and
    did not fall back (16, 1, 0), 3 launches. Child process 2.0 s."""
    _child("contig", 900)


def test_raw_tiles_over_contiguous_candidates():
    """the same set with MSC_MULTI_NO_DIGEST=1: blocks of 64 + 64 + 2 on k_pair_tiles_multi, 5 launches: sums, classify sums, nine raw
    statistics, flags and counts bit for bit. Child process 1.6 s."""
    _child("contig_tiles", 900)


def test_digest_with_the_distance_from_ranks():
    """MSC_MULTI_NO_GEMM=1, 8-bit bins, 64 and 80 queries x 40 000 slots: 2 chunks of 20 000 a block of 64 (two tiles per step; the kernel's
    name says "emd by ranks", which only that form serves), one for the block of 16. Per child of this kind three calls at 64 queries: the
    nine integer statistics with sums, flags and counts (bit for bit); manhattan beside the two divergence sums under weights_cfg5_k9.txt, a
    model that holds them (the merge pass per query per chunk: the two columns and the sums to the oracle's tolerances, flags equal but
    beside a sum within 1e-10 of 0 -- 0 such flags printed on an MI355X in all four children); sim_mm and rre_k_r (the group pass per query
    per chunk: they came out bit-equal and are asserted so). Child process 2.3 s."""
    _child("digest", 600)


def test_digest_with_its_own_prefix_half():
    """... and MSC_MULTI_NO_RANKS=1: the digest kernel scores the distance itself (name without a distance clause). Child process 2.3 s."""
    _child("digest_prefix", 600)


def test_ring_over_32_bit_bins():
    """MSC_MULTI_NO_DIGEST=1, 32-bit bins: 3 chunks of 13 334 a block of 64, 4 launches of the call of 80. Child process 2.6 s."""
    _child("ring", 600)


def test_raw_tiles_over_16_bit_bins():
    """MSC_MULTI_NO_DIGEST=1, 16-bit bins: 2 chunks of 20 000 a block of 64, 3 launches of the call of 80. Child process 2.7 s."""
    _child("tiles", 600)


def test_group_records_cap_with_no_switch_set():
    """sim_mm and rre_k_r wanted of 128 and 130 queries x 40 000 slots in the default environment: 2 chunks of 20 000 for the block of 128
    (8-bit k = 9: the list form of the group pass; 16-bit k = 7: the dense group kernels), both on the matrix cores; 3 launches of the
    130-query call. Sums, classify sums, flags, counts and the two statistics bit for bit against the one-chunk call. Child process 6.2 s,
    most of it the oracle's sim_mm (16 ms a pair at k = 9 on one core)."""
    _child("groups", 600)
