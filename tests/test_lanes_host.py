"""CPU: lanes_plan (epgpy_amd/csrc/epgx_planner.cpp) -- which cut record lists the one-voxel-per-lane variant of the growing launch
takes, every reason it refuses one for, and the live count L for 1 .. 31 echoes and probed / unprobed mixes -- compiled with the
host compiler alone and run through tests/host/lanes_check.cpp.  The program prints one line per check and exits non-zero at the
first failure."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "epgpy_amd", "csrc")


def test_lanes_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lanes_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe,
                           os.path.join(HERE, "host", "lanes_check.cpp"), os.path.join(CSRC, "epgx_planner.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.rstrip().endswith("lanes_check: all checks passed")
