"""ds2i_amd/csrc/host_parallel.hpp: the one host thread pool of the build side ("fn for every index, indices drawn off a
counter"). tests/host_parallel_check.cpp is a stand-alone program (its own main, no HIP, nothing loaded into Python) that holds
the pool to its contract; this test compiles it with the host compiler and runs it. The same source builds and runs clean with
-fsanitize=thread and with -fsanitize=address,undefined (CHANGELOG.md says when that was last done)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = (1, 3, 16)


def host_compiler():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:  # the compiler the library itself is built with (ds2i_amd/build.py)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    return cxx


def test_parallel_for_contract(tmp_path):
    exe = str(tmp_path / "host_parallel_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(HERE, "host_parallel_check.cpp"), "-o", exe],
                   check=True, timeout=120)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.splitlines()
    assert not [l for l in lines if l.startswith("FAIL")]
    assert lines[-1] == "host_parallel: all checks passed"
    # every case the contract names was run: each index once for n in {0, 1, threads - 1, threads + 1, 1000}, with and
    # without the caller taking part; an exception (std, bad_alloc, not a std::exception) reaching the caller
    for threads in THREADS:
        for caller in (0, 1):
            for n in (0, 1, threads - 1, threads + 1, 1000):
                assert "visits n=%d threads=%d caller_takes_part=%d" % (n, threads, caller) in lines
            assert lines.count("throws n=1000 threads=%d caller_takes_part=%d" % (threads, caller)) == 2
            assert "throws n=%d threads=%d caller_takes_part=%d" % (threads + 1, threads, caller) in lines
