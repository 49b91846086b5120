"""CPU: run analysis (epgpy_amd/csrc/epgx_run_check.cpp: the checks of epgx_run, epgx_kernel_for and the tiled entry points, the
route of a range with its kernel name, the tile shape and the slab rule) compiled with the host compiler alone and run through
tests/host/run_check.cpp -- the C++ that ships, on a machine without a GPU.  The program prints one line per check and exits
non-zero at the first failure; `make -C tests/host asan` builds it with the sanitizers (run by hand, on the CPU)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "epgpy_amd", "csrc")


def test_run_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "run_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe,
                           os.path.join(HERE, "host", "run_check.cpp"), os.path.join(CSRC, "epgx_run_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.rstrip().endswith("run_check: all checks passed")
