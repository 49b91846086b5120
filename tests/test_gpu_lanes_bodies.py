"""The record bodies of rows_grow_lanes_kernel (epgx_grow_lanes_kernels.hip.h): the bodies specialised on a record's shifts and
chain kinds run the cells of the generic body in blocks, on the same operands and in the same order, so the probes must be those
of the generic body BIT FOR BIT.  EPGX_LANES_BODY is read once per process: both sides run in child processes
(tests/lanes_body_cases.py: the cases of tests/lanes_cases.py and the edges of the blocks and of the deck), one with
EPGX_LANES=2 EPGX_LANES_BODY=0, one with EPGX_LANES=2 and EPGX_TRACE, whose `variant lanes` line names the bodies."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg
from tests import lanes_body_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("EPGX_LANES", "EPGX_LANES_BODY", "EPGX_TRACE", "EPGX_LANES_CASES")


def child(out, **env):
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lanes_body_cases.py"), out], check=True, env=dict(base, **env),
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
    d = tmp_path_factory.mktemp("lanes_bodies")
    generic, gtraces = child(str(d / "generic.npz"), EPGX_LANES="2", EPGX_LANES_BODY="0", EPGX_TRACE="1")
    bodies, traces = child(str(d / "bodies.npz"), EPGX_LANES="2", EPGX_TRACE="1")
    return generic, gtraces, bodies, traces


def named(trace):
    """the bodies the `variant lanes` lines of a case name"""
    return re.findall(r"run: variant lanes \(one voxel per lane\): L = \d+, .*, body (\S+)$", trace, re.M)


def test_bodies_are_bit_identical_to_the_generic_body(both):
    generic, _, bodies, _ = both
    all_cases = lanes_body_cases.cases(epg)
    assert set(all_cases) == set(generic.files) == set(bodies.files)
    for name in all_cases:
        assert bodies[name].shape == generic[name].shape and np.array_equal(bodies[name], generic[name]), name


def test_trace_names_the_body_of_every_launch(both):
    _, gtraces, _, traces = both
    specialised = 0
    for name, (_, _, _, variant, body) in lanes_body_cases.cases(epg).items():
        seen = traces[name]
        if variant == "lanes" and "rows_grow_kernel" in seen:
            assert named(seen) == [body], (name, seen)
            assert named(gtraces[name]) == [lanes_body_cases.GENERIC], (name, gtraces[name])
            specialised += body != lanes_body_cases.GENERIC
        else:                                 # (no growing launch, or one the variant is refused for)
            assert "variant lanes" not in seen and "variant lanes" not in gtraces[name], (name, seen)
    # not vacuous: the launches that tests/test_gpu_lanes.py knows to take the variant run the blocked echo body, the unfused
    # pairs and the folded MRF records the fallback
    print({name: named(t) for name, t in traces.items() if named(t)})
    assert specialised >= 5
    for name in ("mse_9x8_20", "mse_9x8_23", "mse_5x4x4_20", "mse_1x3_16", "unprobed_tail"):
        assert named(traces[name]) == [lanes_body_cases.ECHO], (name, traces[name])
    for name in ("unfused_20", "mrf_40"):
        assert named(traces[name]) == [lanes_body_cases.GENERIC], (name, traces[name])
