"""CPU: plan analysis (epgpy_amd/csrc/epgx_plan_check.cpp: the checks of epgx_plan_create, the grid geometry, the zero patterns
and snaps, the recipes, the layout of the log tables) compiled with the host compiler alone and run through
tests/host/plan_check.cpp -- the C++ that ships, on a machine without a GPU.  The program prints one line per check and exits
non-zero at the first failure; `make -C tests/host asan` builds it with the sanitizers (run by hand, on the CPU)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "epgpy_amd", "csrc")


def test_plan_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "plan_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(HERE, "host", "plan_check.cpp"), os.path.join(CSRC, "epgx_plan_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.rstrip().endswith("plan_check: all checks passed")
