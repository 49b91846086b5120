"""CPU: the argument checks of the signal consumers (epgpy_amd/csrc/epgx_signal_check.cpp: everything epgx_signal_crlb, _crlb_grad,
_norms(_c64), _match(_c64), _refine, _component_gram, _nnls, _nnls_chi2, _gram and _project decide before they need the device --
NULL and alignment, ranges, overflow-safe extents, the split rule, the LDS chunks and the scratch lengths) compiled with the host
compiler alone and run through tests/host/signal_check.cpp -- the C++ that ships, on a machine without a GPU.  The program prints
one line per check and exits non-zero at the first failure; `make -C tests/host asan` builds it with the sanitizers (run by hand,
on the CPU)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "epgpy_amd", "csrc")


def test_signal_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "signal_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe,
                           os.path.join(HERE, "host", "signal_check.cpp"), os.path.join(CSRC, "epgx_signal_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.rstrip().endswith("signal_check: all checks passed")
