"""ds2i_amd/csrc/unit_cut.hpp: how cut_units cuts a conjunctive query into work units (equal parts, or parts that taper from a few
large ones to the equal part). tests/unit_cut_check.cpp is a stand-alone program (its own main, no HIP) that sweeps block counts from
1 to 2^25, costs from 0 to 10^9 targets, ratios and caps and checks exact cover, non-increasing sizes, the smallest part, the bounds on
the part count, equality with the equal cut at ratio 1 / cap = target, and determinism. This test compiles it with the host compiler
under -fsanitize=address,undefined and runs it as a child process."""
import os
import subprocess

from test_host_parallel_cpu import host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


def test_unit_cut_properties(tmp_path):
    exe = str(tmp_path / "unit_cut_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "unit_cut_check.cpp"), "-o", exe], check=True, timeout=120)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("unit_cut:"), run.stdout
