"""Sizing of the radix partition (no GPU needed): what mdb_partition_arena_bytes, mdb_partition_level0_arena_bytes,
mdb_partition_raw_arena_bytes, mdb_sort_pass_hist_words and mdb_partition_w32_applies return over a grid of requests, printed by a
stand-alone host program (tests/partition_layout_main.cpp, linked against the built library) and compared with
tests/golden/partition_layout.json.  The operators reserve their arena by these figures before they run: a change of the partition's
host code that moves one of them shows up here as a diff, row by row."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "partition_layout.json")


def _hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def layout_rows(workdir):
    """compile the program as host C++ (ROCm headers on the include path, no device code, no sanitizer), run it, return its rows"""
    from midoridb_amd.lib import library_path
    hipcc = _hipcc()
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    lib = library_path()
    assert os.path.exists(lib), lib
    exe = os.path.join(str(workdir), "partition_layout")
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "midoridb_amd", "csrc"),
           os.path.join(ROOT, "tests", "partition_layout_main.cpp"), "-x", "none", lib,
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib"), "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout)["rows"]


def test_sizing_functions_return_the_recorded_figures(tmp_path):
    if not _hipcc():
        pytest.skip("needs hipcc")
    got = layout_rows(tmp_path)
    with open(GOLDEN) as f:
        want = json.load(f)["rows"]
    assert len(got) == len(want), (len(got), len(want))
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, (len(diff), diff[:10])
    # the grid is the one the golden file was recorded over: every function, every table size
    assert {r[0] for r in got} == {"choose_bits", "sort_pass_hist_words", "w32_applies", "arena_bytes", "raw_arena_bytes", "level0_arena_bytes"}
    assert {r[1] for r in got} == {0, 1, 4095, 4096, 4097, 393215, 393217, 1 << 20, (1 << 21) + 5, (1 << 25) - 1, 1 << 25, 10**8, (1 << 32) - 2}
