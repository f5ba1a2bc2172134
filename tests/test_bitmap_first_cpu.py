"""RmwLevels::bitmap_first (ds2i_amd/csrc/abi_structs.hpp): where k_ranked_stream fetches list 1's bitmap byte ahead instead of its
hint byte. tests/bitmap_first_check.cpp is a stand-alone program (its own main, no HIP) that sweeps (n, num_docs, shift) and
compares the rule with RmwLevels' own geometry; this test compiles it with the host compiler and runs it."""
import os
import subprocess

from test_host_parallel_cpu import host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


def test_bitmap_first_rule(tmp_path):
    exe = str(tmp_path / "bitmap_first_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "bitmap_first_check.cpp"), "-o", exe], check=True, timeout=120)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("bitmap_first:"), run.stdout
