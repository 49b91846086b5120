"""rows_grow_lanes_kernel_odd (epgx_grow_lanes_odd_kernels.hip.h): an echo train with one voxel per lane, computing only the orders
whose parity reaches an echo, all of them in registers.  Its cells are the odd cells of rows_grow_lanes_kernel<NSP, true> -- the
same chains on the same operands -- so its probes must be that kernel's BIT FOR BIT.  Both sides run tests/lanes_odd_cases.py
(the cases of tests/lanes_train_cases.py and three more probe patterns) in a child process with EPGX_LANES=2 and EPGX_TRACE=1:
one with EPGX_LANES_ODD=2 (the kernel wherever the list allows it), one with EPGX_LANES_ODD=0 (never).  A list that is
LanesPlan::odd must trace the kernel's own line and no `variant lanes (one voxel per lane)` line; every other list (a lone
S(+1) behind the excitation, lists that are no trains) must trace what it traces without the kernel."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg
from tests import lanes_odd_cases, lanes_train_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("EPGX_LANES", "EPGX_LANES_BODY", "EPGX_LANES_TRAIN", "EPGX_LANES_ODD", "EPGX_TRACE", "EPGX_LANES_CASES")
# a probe behind every other echo: the planner does not make a growing launch at 64 orders of this list (its records alternate),
# so neither kernel runs it -- the case stays for the agreement of the two sides
NO_GROW = lanes_train_cases.NO_GROW + ("every_other_echo_20",)
OLD_LINE = "run: variant lanes (one voxel per lane)"
NEW_LINE = re.compile(r"run: variant lanes-odd \(one voxel per lane, odd orders only\): L = (\d+), kernel rows_grow_lanes_kernel_odd "
                      r"\((\d+) cells of 2 orders\), state in (\d+) VGPRs, 0 bytes of LDS per wave, (\d+) shifts before the last probe$", re.M)


def child(out, **env):
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lanes_odd_cases.py"), out], check=True,
                         env=dict(base, EPGX_TRACE="1", EPGX_LANES="2", **env), cwd=ROOT, timeout=600, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    traces, name = {}, None
    for line in run.stderr.splitlines():
        if line.startswith("[case] "):
            name = line[7:]
            traces[name] = []
        elif name is not None:
            traces[name].append(line)
    return np.load(out), {k: "\n".join(v) for k, v in traces.items()}


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    d = tmp_path_factory.mktemp("lanes_odd")
    return {"odd": child(str(d / "odd.npz"), EPGX_LANES_ODD="2"), "off": child(str(d / "off.npz"), EPGX_LANES_ODD="0")}


def test_odd_kernel_is_bit_identical(sides):
    signals, _ = sides["odd"]
    ref, _ = sides["off"]
    all_cases = lanes_odd_cases.cases(epg)
    assert set(all_cases) == set(signals.files) == set(ref.files) and len(all_cases) == len(lanes_train_cases.cases(epg)) + 3
    for name, case in all_cases.items():
        assert signals[name].shape == ref[name].shape and np.array_equal(signals[name], ref[name]), name
        if lanes_odd_cases.is_odd(case):     # (behind a lone S(+1) every probe reads the other parity: those signals are zero)
            assert np.abs(ref[name]).max() > 1e-3, name


def test_trace_names_the_kernel_of_every_launch(sides):
    odd_launches, others = [], []
    for name, case in lanes_odd_cases.cases(epg).items():
        on, off = sides["odd"][1][name], sides["off"][1][name]
        lanes_lines = [line for line in off.splitlines() if OLD_LINE in line]
        if "rows_grow_kernel" not in off:        # no growing launch at 64 orders: nothing to select on either side
            assert name in NO_GROW and "run: variant" not in on and "run: variant" not in off, name
            continue
        assert len(lanes_lines) == 1 and f"kernel {case[3]} (deck" in lanes_lines[0], (name, off)
        assert not NEW_LINE.search(off), (name, off)
        got = NEW_LINE.findall(on)
        print(name, lanes_odd_cases.is_odd(case), got)
        if lanes_odd_cases.is_odd(case):
            assert len(got) == 1 and OLD_LINE not in on, (name, on)
            L, cells, vgprs, rem0 = map(int, got[0])
            assert cells == 12 and vgprs == 144 and L <= 2 * cells and rem0 % 2 == 0, (name, got)
            assert f"L = {L}, kernel train" in lanes_lines[0] and f"{rem0} shifts before the last probe" in lanes_lines[0], (name, off)
            odd_launches.append(name)
        else:                                    # the old line, unchanged
            assert not got and [line for line in on.splitlines() if OLD_LINE in line] == lanes_lines, (name, on)
            others.append(name)
    print("odd:", odd_launches, "others:", others)
    # the lone-shift heads and the lists that are no trains stay; the trains at the block edges, at the cap, on two index
    # spaces, behind two head records, with an unprobed tail and with unprobed echoes between probed ones move
    assert {"odd_lead_20", "odd_lead_tail_10", "mse_5x4x4_17", "unfused_17", "mrf_40"} <= set(others)
    want = {f"mse_9x8_{n}" for n in lanes_train_cases.ECHOES if n not in lanes_train_cases.SHORT}
    want |= {f"tail_{n}" for n in lanes_train_cases.SHORT} | {"exc_b1_5x4x4_17", "two_heads_16", "unprobed_tail_9", "unprobed_middle_20"}
    assert want <= set(odd_launches)
    # 5 probed + 5 unprobed + 10 probed echoes: the window is that of all 20, and 15 rows come out
    assert int(NEW_LINE.findall(sides["odd"][1]["unprobed_middle_20"])[0][0]) == 21 and sides["odd"][0]["unprobed_middle_20"].shape[0] == 15
    for necho in lanes_train_cases.ECHOES:       # the live counts: L = echoes + 1, up to the cap of 24
        name = f"tail_{necho}" if necho in lanes_train_cases.SHORT else f"mse_9x8_{necho}"
        assert int(NEW_LINE.findall(sides["odd"][1][name])[0][0]) == necho + 1, name
