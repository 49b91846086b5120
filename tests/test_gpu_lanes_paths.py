"""The three one-voxel-per-lane kernels of the growing launch -- `train` (rows_grow_lanes_kernel<NSP, true>), `any list`
(rows_grow_lanes_kernel<NSP, false>) and `lanes-odd` (rows_grow_lanes_kernel_odd<NSP, 12>), NSP 0 / 1 / 2 / 4 each -- against the
extended-precision recurrence PER RECORD, on grids with a third workgroup and a ragged last one, on voxel sub-ranges, and under
the default routing at the threshold of 2^19 voxels (cases, floors and checks: tests/lanes_path_cases.py; the floors are kept
honest by tests/test_lanes_paths_host.py).

choose_kernel names the family rows_grow_kernel<NSP> only; the launcher (epgx_launch_grow.h) picks the variant and says so in one
EPGX_TRACE line.  The library reads its knobs once per process, so every side is ONE child process that runs
tests/lanes_path_cases.py with EPGX_TRACE=1; the children run one after another, and once one of them has failed or run into
its time limit no further child is started: the remaining tests fail without touching the device.

  (a) every case on every side: the trace line (family, variant, kernel, L) FIRST, then
      max_vox|gpu[r] - ref[r]| <= 16 floor max_vox|ref[r]| for every record r; records of zeros exactly zero;
  (b) voxel sub-ranges [37, 107) and [64, 128) through _lib.run into a buffer over the whole grid filled with 7 + 7i: the
      columns of the range are the bits of the full launch, everything else is still 7 + 7i;
  (c) no knob set: 1024 x 512 = 2^19 voxels trace lanes-odd / train / any list, 2^19 - 1 voxels trace the rows variant; every
      column is the bits of the column with the same parameters of the small launch of (a)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lanes_path_cases as lp
from tests.lanes_path_cases import CASES, SIDES, SUB_CASES, SUBRANGES, THRESHOLD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = {"default": 180}          # seconds per child: 33 small launches and 16 sub-range launches (120; a second or two when warm) / and the four big launches


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest per-record |gpu - extended reference| / max|ref record| over the case's float64 floor, per kernel:",
          {k: float(f"{v:.3g}") for k, v in sorted(lp.RATIO.items())})


_FAULT = []          # the first child that failed: nothing more is started on the device after it


def guarded(fn):
    """run device work; once a child process has failed, every later test fails before it touches the device"""
    if _FAULT:
        pytest.fail(f"not run: an earlier child process failed ({_FAULT[0]!r})")
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as exc:
        _FAULT.append(exc)
        raise


_REF, _SIDE = {}, {}


def reference(name):
    if name not in _REF:
        _REF[name] = lp.reference(name)
    return _REF[name]


def side(name, tmp_path_factory):
    """(signals, {launch: trace lines}, path of the .npz) of one side: its child process runs once"""
    if name not in _SIDE:
        out = str(tmp_path_factory.mktemp("lanes_paths") / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in lp.KNOBS}
        env.update(SIDES[name], EPGX_TRACE="1")
        env["EPGX_PATHS_THRESHOLD" if name == "default" else "EPGX_PATHS_SUBRANGE"] = "1"

        def run():
            done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lanes_path_cases.py"), out], env=env, cwd=ROOT,
                                  timeout=TIMEOUT.get(name, 120), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if done.returncode != 0:
                raise RuntimeError(f"side {name}: exit status {done.returncode}: {done.stderr[-2000:]}")
            traces, launch = {}, None
            for line in done.stderr.splitlines():
                if line.startswith("[case] "):
                    launch = line[7:]
                    traces[launch] = []
                elif launch is not None:
                    traces[launch].append(line)
            return dict(np.load(out)), {k: "\n".join(v) for k, v in traces.items()}, out
        _SIDE[name] = guarded(run)
    return _SIDE[name]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("which", list(SIDES))
def test_records(which, name, tmp_path_factory):
    signals, traces, _ = side(which, tmp_path_factory)
    c = CASES[name]
    kernel = lp.kernel_on(c, which)
    lp.check_trace(traces[name], kernel, c["L"], c["nsp"])                 # BEFORE the comparison
    want = reference(name)
    assert signals[name].shape == want.shape, (signals[name].shape, want.shape)
    lp.check_case(f"{kernel}<{c['nsp']}>", name, signals[name], want)


@pytest.mark.parametrize("vox0, nvox", SUBRANGES)
@pytest.mark.parametrize("name", SUB_CASES)
@pytest.mark.parametrize("which", [s for s in SIDES if s != "default"])
def test_voxel_subranges(which, name, vox0, nvox, tmp_path_factory):
    signals, traces, _ = side(which, tmp_path_factory)
    c = CASES[name]
    launch = f"sub_{vox0}_{nvox}:{name}"
    lp.check_trace(traces[launch], lp.kernel_on(c, which), c["L"], c["nsp"])
    assert vox0 + nvox < int(np.prod(lp.grid_of_case(c)))                   # (the range ends inside the grid: columns behind it)
    lp.check_subrange(signals[launch], signals[name], vox0, nvox)


@pytest.mark.parametrize("name", list(THRESHOLD))
def test_default_routing_at_the_threshold(name, tmp_path_factory):
    _, traces, out = side("default", tmp_path_factory)
    small, big, kernel = THRESHOLD[name]
    c = CASES[small]
    nvox = int(np.prod(big))
    assert nvox == lp.LANES_MIN_VOXELS - (kernel == "rows")
    lp.check_trace(traces[name], kernel, c["L"], c["nsp"])
    # the small launch on the same kernel (the rows variant: the default side itself)
    held = {lp.ODD: "odd", lp.TRAIN: "lanes", lp.ANY: "lanes", "rows": "default"}[kernel]
    assert lp.kernel_on(c, held) == kernel
    small_signals = side(held, tmp_path_factory)[0][small]
    path = f"{out}.{name}.npy"
    got = np.load(path, mmap_mode="r")
    try:
        assert got.shape == (small_signals.shape[0],) + tuple(big)
        lp.check_tiling(got, small_signals)
    finally:
        del got
        os.remove(path)
