"""CPU: the host side of rows_grow_lanes_kernel_odd, the echo-train kernel that computes the orders of one parity alone.

tests/host/lanes_odd_check.cpp -- LanesPlan::odd and lanes_odd_selected (epgpy_amd/csrc/epgx_planner.{h,cpp}): plain trains of
1 .. 23 echoes are `odd`, probed everywhere or not; a shifting head record (an odd number of shifts before the last probe), a
list that is no train and an MRF list are not; EPGX_LANES_ODD = 0 / 1 / 2 on both sides of LANES_MIN_VOXELS; `odd` itself does
not follow the knobs.

tests/host/lanes_odd_cells_check.cpp -- the kernel's cell loop (epgpy_amd/csrc/epgx_lanes_odd_cells.h), compiled for the host
with AddressSanitizer and UBSan: every window of every train up to L = 24 at every capacity that holds it stays inside the
state, and the probe equals that of the full record of rows_grow_lanes_kernel bit for bit.

Both are stand-alone programs that print one line per check and exit non-zero at the first failure."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "epgpy_amd", "csrc")


def build_and_run(tmp_path, name, sources, flags):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-o", exe] + flags + sources)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.rstrip().endswith(f"{name}: all checks passed")


def test_lanes_odd_check(tmp_path):
    build_and_run(tmp_path, "lanes_odd_check", [os.path.join(HERE, "host", "lanes_odd_check.cpp"), os.path.join(CSRC, "epgx_planner.cpp")],
                  ["-O1"])


def test_lanes_odd_cells_check_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "lanes_odd_cells_check", [os.path.join(HERE, "host", "lanes_odd_cells_check.cpp")],
                  ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
