"""The integer cut of a folded block (csrc/msc_fold_reject.h) without a device: tests/fold_reject_check.cpp, built with the address
and undefined-behaviour sanitizers, holds the certificate to an FP64 evaluation written from the reference's formulas -- over random models and
the two golden `fast` weights files, no pair under a cut may be close --, measures how much of a cfg2-shaped sample the cut covers (the gate
the kernels were built behind: at least 90 % of the unrelated pairs under their query's cut), and writes the cuts and rejected pairs of a small set
for the oracle to judge in both argument orders. And the switch through the public layers."""
import os
import re
import subprocess

import numpy as np
import pytest

from golden_util import weights_text
from meshclust2_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS, PAIRS = 64, 1000000          # random models, and the pairs under a cut each is held to (a model that hardly ever gets a cut ends short)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("fold_reject") / "fold_reject_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "fold_reject_check.cpp"), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    return str(out)


def _sequences(path, seed, n, family):
    seqs = synth.families(seed, n, 1000, family=family)[0]
    with open(path, "wb") as f:
        f.write(b"\n".join(seqs) + b"\n")
    return seqs


def test_no_certified_pair_is_close(exe):
    """at least 10^6 drawn pairs under a cut per model, over at least 50 random models and the two golden files: none close in FP64"""
    r = subprocess.run([exe, "soundness", str(MODELS), str(PAIRS), os.path.join(GOLDEN, "weights_k9_u32.txt"), os.path.join(GOLDEN, "weights_k8_u16.txt")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = r.stdout.decode()
    print(text[-3000:])
    assert r.returncode == 0 and "fold reject soundness ok" in text, text[-6000:]
    assert "edge cases without a certificate: 0 wrong" in text          # a zero length in range, a sum below 4^k, 2^31, an empty range, NaN, no image, another statistic
    m = re.search(r"soundness: (\d+) pairs under a cut, (\d+) models with a cut, (\d+) models with %d pairs or more.* (\d+) certified and close" % PAIRS, text)
    assert m and int(m.group(4)) == 0
    assert int(m.group(3)) >= 50 and int(m.group(1)) >= 50 * PAIRS


def test_the_gate_on_a_cfg2_shaped_sample(exe, tmp_path):
    """2 000 synthetic 1 kb sequences in families of 20, k = 9, 32-bit bins, folded 16-to-1 on the CPU, tests/golden/weights_k9_u32.txt: the share of
    unrelated pairs with P1' + P2' at most their query's cut (every 20th sequence a query), and every rejected pair not close by its true reductions"""
    path = tmp_path / "cfg2.txt"
    _sequences(path, 20260001, 2000, 20)
    share = {}
    for order in (0, 1):
        r = subprocess.run([exe, "sample", str(path), os.path.join(GOLDEN, "weights_k9_u32.txt"), "9", "32", str(order), "20", "20"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        text = r.stdout.decode()
        print(text)
        assert r.returncode == 0 and "fold reject sample ok" in text, text
        share[order] = float(re.search(r"^gate ([0-9.]+)$", text, re.M).group(1))
    print("gate: unrelated pairs under their query's cut, candidate first %.4f, query first %.4f" % (share[0], share[1]))
    assert min(share.values()) >= 0.90


def _shifted(text, by):
    """the classification block of a weights file with its intercept moved (the line after the first `n_combos:`)"""
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("n_combos:")) + 1
    lines[at] = repr(float(lines[at]) + by)
    return "\n".join(lines) + "\n"


def test_rejected_pairs_against_the_oracle(exe, tmp_path, oracle):
    """400 sequences in families of four at k = 8, 16-bit bins, the golden k = 8 model with its intercept moved by -2 (as trained, every pair of this
    set is close and no row gets a cut): for every pair, U <= T(q) implies the oracle's flag is 0, in both argument orders. The oracle's candidate-first
    flags of all 400 x 400 pairs are computed once: f(query, candidate) is their transpose."""
    n, k, dtype = 400, 8, 16
    path, wpath = tmp_path / "fam4.txt", tmp_path / "weights.txt"
    seqs = _sequences(path, 20260002, n, 4)
    text = _shifted(weights_text("weights_k8_u16.txt"), -2.0)
    wpath.write_text(text)
    pred = oracle.predictor(text)
    hists = [oracle.hist(s, k, dtype) for s in seqs]
    try:
        cand_first = np.stack([oracle.get_close(pred, 1e-9, hists[q], hists, omp=True)[0] for q in range(n)])          # [q][c] = f(candidate c, query q)
    finally:
        for h in hists:
            oracle.lib().orc_hist_free(h)
    assert cand_first.any() and not cand_first.all()
    for order, flags in ((0, cand_first), (1, cand_first.T)):
        out = tmp_path / ("cuts%d.bin" % order)
        r = subprocess.run([exe, "sample", str(path), str(wpath), str(k), str(dtype), str(order), "4", "1", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()
        raw = np.fromfile(out, dtype=np.uint8)
        cuts = raw[:4 * n].view(np.int32)
        rejected = raw[4 * n:].reshape(n, n).astype(bool)
        print("order %d: %d rows with a cut, %d of %d pairs rejected, %d close pairs" % (order, int((cuts >= 0).sum()), int(rejected.sum()), n * n, int(flags.sum())))
        assert rejected.any()
        assert not (flags.astype(bool) & rejected).any()


def test_the_switch_is_carried_through_the_layers():
    text = open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()
    assert re.search(r"\bint\s+msc_set_fold_reject\s*\(\s*msc_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", text)
    assert re.search(r"\bint\s+msc_last_fold_reject\s*\(", text)
    from meshclust2_amd import _capi, api
    assert "msc_set_fold_reject" in _capi.PROTOTYPES and "msc_last_fold_reject" in _capi.PROTOTYPES
    assert hasattr(api.Context, "set_fold_reject") and hasattr(api.Context, "last_fold_reject")
    host = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"void\s+set_fold_reject\s*\(\s*bool\s+on\s*\)\s*\{\s*check\(msc_set_fold_reject\(", host)
