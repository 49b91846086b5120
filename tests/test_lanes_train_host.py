"""CPU: LanesPlan::train and lanes_train_selected (epgpy_amd/csrc/epgx_planner.{h,cpp}) -- which record lists of the
one-voxel-per-lane variant run its kernel without a generic record body: fused trains do; unfused trains, MRF lists, a train
with a record without a body behind its first shift do not; records of any kind before the first shift do not matter; and the
knobs EPGX_LANES_TRAIN / EPGX_LANES_BODY keep a train on the other kernel without changing what the plan says about the list.
Compiled with the host compiler alone and run through tests/host/lanes_train_check.cpp, which prints one line per check and
exits non-zero at the first failure."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "epgpy_amd", "csrc")


def test_lanes_train_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lanes_train_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe,
                           os.path.join(HERE, "host", "lanes_train_check.cpp"), os.path.join(CSRC, "epgx_planner.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.rstrip().endswith("lanes_train_check: all checks passed")
