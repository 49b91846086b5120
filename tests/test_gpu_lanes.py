"""The one-voxel-per-lane variant of the growing launch (rows_grow_lanes_kernel; selection: epgx_launch_grow.h, eligibility:
lanes_plan in epgx_planner.cpp).  It computes the live orders only and issues the chains of the rows cells on plain registers,
so its signals must be those of the rows variant BIT FOR BIT, and agree with the oracle as everywhere else.

The library reads EPGX_LANES once per process, at its first launch, and this process may have launched already: both sides run
in child processes (tests/lanes_cases.py), one with EPGX_LANES=0, one with EPGX_LANES=2 and EPGX_TRACE, whose stderr says
which variant every launch took."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg
from oracle import epg_numpy as onp
from tests import lanes_cases

pytestmark = pytest.mark.gpu
TOL = 1e-12                                    # (tests/test_gpu_reach.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, tol=TOL):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    assert err <= tol * max(1.0, float(np.max(np.abs(b))) if b.size else 1.0), err


def child(out, **env):
    base = {k: v for k, v in os.environ.items() if k not in ("EPGX_LANES", "EPGX_TRACE")}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lanes_cases.py"), out], check=True, env=dict(base, **env),
                         cwd=ROOT, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    traces, name = {}, None
    for line in run.stderr.splitlines():
        if line.startswith("[case] "):
            name = line[7:]
            traces[name] = []
        elif name is not None:
            traces[name].append(line)
    return np.load(out), {k: "\n".join(v) for k, v in traces.items()}


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    d = tmp_path_factory.mktemp("lanes")
    rows, _ = child(str(d / "rows.npz"), EPGX_LANES="0")
    lanes, traces = child(str(d / "lanes.npz"), EPGX_LANES="2", EPGX_TRACE="1")
    return rows, lanes, traces


def test_lanes_is_bit_identical_to_rows(both):
    rows, lanes, traces = both
    all_cases = lanes_cases.cases(epg)
    assert set(all_cases) == set(rows.files) == set(lanes.files) and len(all_cases) >= 3 * len(lanes_cases.ECHOES) + 9
    for name, (_, _, _, variant) in all_cases.items():
        seen = traces[name]
        if "rows_grow_kernel" in seen:         # (a launch that is not a growing one -- the shortest trains, 16 orders -- has nothing to select)
            assert f"run: variant {variant}" in seen, (name, seen)
        else:
            assert "run: variant" not in seen, (name, seen)
        assert lanes[name].shape == rows[name].shape and np.array_equal(lanes[name], rows[name]), name
    # the comparison is not vacuous: the trains the variant is for do take it, with the live counts the planner promises
    for name, L in (("mse_9x8_20", 21), ("mse_9x8_23", 24), ("mse_5x4x4_20", 21), ("mse_1x3_16", 17), ("unprobed_tail", 10)):
        assert f"run: variant lanes (one voxel per lane): L = {L}," in traces[name], (name, traces[name])
    # (every_other_echo does not fold into a growing list -- it runs rows_kernel on either side -- and stays for the agreement)
    for name in ("unfused_20", "mrf_40"):
        assert "run: variant lanes" in traces[name], (name, traces[name])
    assert "rows_grow_kernel<2>" in traces["mse_5x4x4_20"], traces["mse_5x4x4_20"]


def test_lanes_agrees_with_the_oracle(both):
    _, lanes, _ = both
    for name, (tuples, _, kw, _) in lanes_cases.cases(epg).items():
        options = {k: v for k, v in kw.items() if k != "fuse"}
        try:
            close(lanes[name], onp.simulate(tuples, **options))
        except AssertionError as exc:
            raise AssertionError(f"{name}: {exc}") from None


def test_small_launches_stay_on_rows_by_default(tmp_path):
    """EPGX_LANES=1, set or by default: a 72-voxel launch is far below the threshold and traces the rows variant"""
    for env in ({"EPGX_LANES": "1"}, {}):
        _, traces = child(str(tmp_path / "small.npz"), EPGX_TRACE="1", EPGX_LANES_CASES="mse_9x8_20", **env)
        seen = traces["mse_9x8_20"]
        assert "rows_grow_kernel<1>" in seen and "run: variant rows" in seen and "variant lanes" not in seen, seen
