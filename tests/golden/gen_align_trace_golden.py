#!/usr/bin/env python3
"""Writes tests/golden/align_trace.npz: for every (parameter set, pair) of tests/golden/align_pairs.npz the number of runs of the pair's CIGAR,
the SHA-256 of the runs' little-endian bytes and whether the path is real, all from tests/align_trace_util.py, the numpy restatement of
DESIGN.md 4.6h. Restatement output, not reference code: the generator stops unless the restatement's triples are the reference's own
(align_pairs.npz) and every CIGAR replays to them.

    python tests/golden/gen_align_trace_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import align_trace_util          # noqa: E402
import align_util                # noqa: E402


def main():
    fx = align_util.Fixture()
    firsts, seconds = [fx.seqs[i] for i in fx.first], [fx.seqs[i] for i in fx.second]
    n_sets, n_pairs = len(fx.params), fx.first.size
    runs = np.zeros((n_sets, n_pairs), dtype=np.uint32)
    sha = np.zeros((n_sets, n_pairs, 32), dtype=np.uint8)
    real = np.zeros((n_sets, n_pairs), dtype=np.uint8)
    for s, params in enumerate(fx.params):
        triples, ops, is_real = align_trace_util.trace_many(firsts, seconds, params)
        assert np.array_equal(triples, fx.result[s]), "the restatement's triples are not the reference's"
        for p in range(n_pairs):
            score, columns, same = align_trace_util.replay(ops[p], firsts[p], seconds[p], params)
            assert columns == triples[p, 1] and (params[0] == params[1] or same == triples[p, 2]) and (not is_real[p] or score == triples[p, 0]), (s, p)
            runs[s, p] = len(ops[p])
            sha[s, p] = np.frombuffer(align_trace_util.digest(ops[p]), dtype=np.uint8)
        real[s] = is_real
        print("set", params.tolist(), "runs", int(runs[s].sum()), "not real", int((~is_real).sum()), flush=True)
    np.savez_compressed(align_trace_util.FIXTURE, runs=runs, sha256=sha, real=real)
    print(align_trace_util.FIXTURE, os.path.getsize(align_trace_util.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
