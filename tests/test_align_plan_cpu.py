"""The launch plans of the alignment kernels without a device (csrc/msc_align_plan.h): tests/align_plan_check.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers, plans seeded lists -- lengths at the edges of every LDS class,
a pair past kAlignLdsMax, enough global-carry pairs to cross kAlignScratchRows, half-widths 1, 17, 64, 128, 129, 512, 513 and none; tile
lists at 16 and 256 rows a tile with first sequences of 255, 256 and 257 bytes, borders past one round's budget and a pair whose tiles
alone pass it -- and holds the full and the banded plan to: a permutation of the input, keys that do not decrease, cells that do not increase
inside a key, equal elements in the input's order, launches that tile the list and mix no keys, the LDS of a launch, disjoint carry ranges
within the scratch rows; and a round of tiles to: every tile the windows allow exactly once, in launch stripe + block, start the exclusive
scan, disjoint borders, both budgets or one pair, the list consumed in order. The header itself must compile as plain C++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meshclust2_amd", "csrc")


def test_the_plan_header_is_plain_cpp(tmp_path):
    src = tmp_path / "only_the_header.cpp"
    src.write_text('#include "msc_align_plan.h"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-c", str(src), "-o", str(tmp_path / "only_the_header.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    text = open(os.path.join(CSRC, "msc_align_plan.h")).read()
    assert "#include <hip" not in text and "msc_objects.h" not in text


def test_the_plans_on_seeded_lists_under_sanitizers(tmp_path):
    exe = tmp_path / "align_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        "-I", CSRC, os.path.join(ROOT, "tests", "align_plan_check.cpp"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"align plan ok" in r.stdout, r.stdout.decode()[-2000:]
