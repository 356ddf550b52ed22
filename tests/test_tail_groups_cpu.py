"""msc_tail_groups (csrc/msc_multi_plan.h) without a device: which consecutive folded blocks of a msc_score_multi call share one tail
(msc_set_tail_groups), how many under the cap, the side's budget and the 32-bit pair count, how the call's final groups halve down to one block,
and where each block's arrays lie in the side -- in a stand-alone program built with the address and undefined-behaviour sanitizers. And the
switch through the public layers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_groups_under_sanitizers(tmp_path):
    exe = tmp_path / "tail_groups_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "tail_groups_check.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"tail groups ok" in r.stdout, r.stdout.decode()


def test_the_switch_is_carried_through_the_layers():
    text = open(os.path.join(ROOT, "include", "meshclust2_hip.h")).read()
    assert re.search(r"\bint\s+msc_set_tail_groups\s*\(\s*msc_ctx\s*\*\s*ctx\s*,\s*int\s+cap\s*\)\s*;", text)
    from meshclust2_amd import _capi, api
    assert "msc_set_tail_groups" in _capi.PROTOTYPES
    assert hasattr(api.Context, "set_tail_groups")
    host = open(os.path.join(ROOT, "meshclust2_amd", "host", "meshclust2_host.hpp")).read()
    assert re.search(r"void\s+set_tail_groups\s*\(\s*int\s+cap\s*\)\s*\{\s*check\(msc_set_tail_groups\(", host)
