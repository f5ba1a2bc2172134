"""ds2i_amd/csrc/batch_plan.{hpp,cpp}: the planner of a query batch, host code only. tests/batch_plan_check.cpp is a stand-alone program
(its own main, no HIP, nothing loaded into Python) that plans batches over a fabricated index -- every operator, k class, flag, batch size
at which the planner changes what it does, five kinds of index, two machine sizes -- and holds every plan to what the slot and the
kernels trust of it (tests/batch_plan_check.cpp says what). This test compiles it together with batch_plan.cpp by the host compiler alone
(no ROCm include path) and runs it as a child process: once under -fsanitize=address,undefined, every case with every check, and once
under -fsanitize=thread with --threaded -- the share of the cases that the planning threads take part in (the planner runs on up to 16
pool threads and reuses its vectors from batch to batch): the error cases, the 36 000-query batches and the comparison of digests over
1, 3, 4 and 16 threads. A machine whose thread-sanitizer runtime does not link or start skips that second run only."""
import os
import subprocess

import pytest

from test_host_parallel_cpu import host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = [os.path.join(HERE, "batch_plan_check.cpp"), os.path.join(HERE, "..", "ds2i_amd", "csrc", "batch_plan.cpp")]


def _build(exe, sanitize):
    return subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-pthread"] + sanitize + SOURCES + ["-o", exe],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def _run(exe, at_least, *args):
    run = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(run.stdout[-2000:])
    assert run.returncode == 0, run.stdout[-4000:]
    last = run.stdout.splitlines()[-1]
    assert last.startswith("batch_plan: ") and last.endswith(" plans hold") and int(last.split()[1]) >= at_least, run.stdout[-4000:]


def test_batch_plans_hold_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "batch_plan_check_asan")
    built = _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert built.returncode == 0, built.stdout
    _run(exe, 3000)


def test_batch_plans_hold_under_tsan(tmp_path):
    exe = str(tmp_path / "batch_plan_check_tsan")
    built = _build(exe, ["-fsanitize=thread"])
    if built.returncode != 0 and ("tsan" in built.stdout or "sanitize=thread" in built.stdout):
        pytest.skip("the thread sanitizer's runtime does not link on this machine: " + built.stdout[-300:])
    assert built.returncode == 0, built.stdout
    probe = subprocess.run([exe, "--probe"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    if probe.returncode != 0 and "ThreadSanitizer" in probe.stdout and "batch_plan" not in probe.stdout:
        pytest.skip("the thread sanitizer's runtime does not start on this machine: " + probe.stdout[-300:])
    _run(exe, 200, "--threaded")
