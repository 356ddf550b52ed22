"""The host arithmetic of the Q x M calls without a device (csrc/msc_multi_plan.h): the blocks msc_score_multi cuts a call's queries into --
128 or 64 at a time, a block that declines the matrix cores cut again into sub-blocks of 64, a trailing single query kept -- and the
candidate chunks of a block, in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_plan_and_candidate_chunks_under_sanitizers(tmp_path):
    exe = tmp_path / "multi_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "multi_plan_check.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"multi plan ok" in r.stdout, r.stdout.decode()
