"""The kernel of the one-voxel-per-lane variant that has no generic record body (rows_grow_lanes_kernel<NSP, true>: head records
run one cell, every other record a specialised body, register deck of 16 orders; epgx_grow_lanes_kernels.hip.h).  Its cells, their
operands and their order are those of the kernel it stands in for, so its probes must be those of that kernel BIT FOR BIT --
with its specialised bodies (EPGX_LANES_TRAIN=0), with the generic body everywhere (EPGX_LANES_BODY=0) -- and those of the rows
variant (EPGX_LANES=0).  The knobs are read once per process: every side runs tests/lanes_train_cases.py in a child process,
with EPGX_TRACE, whose `variant lanes` line names the kernel of every launch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg
from tests import lanes_train_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("EPGX_LANES", "EPGX_LANES_BODY", "EPGX_LANES_TRAIN", "EPGX_TRACE", "EPGX_LANES_CASES")
SIDES = {"default": {}, "train_off": {"EPGX_LANES_TRAIN": "0"}, "body_off": {"EPGX_LANES_BODY": "0"}}


def child(out, **env):
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lanes_train_cases.py"), out], check=True,
                         env=dict(base, EPGX_TRACE="1", **env), cwd=ROOT, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
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
    d = tmp_path_factory.mktemp("lanes_train")
    out = {name: child(str(d / f"{name}.npz"), EPGX_LANES="2", **env) for name, env in SIDES.items()}
    out["rows"] = child(str(d / "rows.npz"), EPGX_LANES="0")
    return out


def kernels(trace):
    """(L, kernel, deck, bytes of LDS per wave) of the `variant lanes` lines of a case"""
    found = re.findall(r"run: variant lanes \(one voxel per lane\): L = (\d+), kernel ([a-z ]+) \(deck (\d+)\), (\d+) bytes of LDS per wave, "
                       r".*, body \S+$", trace, re.M)
    return [(int(L), kernel, int(deck), int(lds)) for L, kernel, deck, lds in found]


@pytest.mark.parametrize("other", ["train_off", "body_off", "rows"])
def test_train_kernel_is_bit_identical(sides, other):
    signals, _ = sides["default"]
    ref, _ = sides[other]
    all_cases = lanes_train_cases.cases(epg)
    assert set(all_cases) == set(signals.files) == set(ref.files) and len(all_cases) >= len(lanes_train_cases.ECHOES) + 6
    for name in all_cases:
        assert signals[name].shape == ref[name].shape and np.array_equal(signals[name], ref[name]), (name, other)


def test_trace_names_the_kernel_of_every_launch(sides):
    trains = 0
    for name, (_, _, _, kernel) in lanes_train_cases.cases(epg).items():
        got = kernels(sides["default"][1][name])
        print(name, got)
        if "rows_grow_kernel" not in sides["default"][1][name]:
            # trains of up to 15 echoes stay within 32 orders: no growing launch at 64, nothing to select (they stay for the
            # agreement; the tail_<n> cases bring their windows to the kernel)
            assert name in lanes_train_cases.NO_GROW and all("run: variant" not in side[1][name] for side in sides.values()), name
            continue
        assert len(got) == 1 and got[0][1] == kernel, (name, sides["default"][1][name])
        L, _, deck, lds = got[0]
        assert deck == (lanes_train_cases.DECK if kernel == lanes_train_cases.TRAIN else 14), (name, got)
        assert lds == 48 * 64 * max(L - deck, 0), (name, got)        # the slots above the deck of the kernel that runs
        trains += kernel == lanes_train_cases.TRAIN
        for other in ("train_off", "body_off"):                      # either knob keeps every list on the kernel with the generic body
            assert [k[1:3] for k in kernels(sides[other][1][name])] == [(lanes_train_cases.ANY, 14)], (name, other, sides[other][1][name])
        assert "variant lanes" not in sides["rows"][1][name], (name, sides["rows"][1][name])
    want = [name for name, case in lanes_train_cases.cases(epg).items() if case[3] == lanes_train_cases.TRAIN]
    assert trains == len(want) - len(lanes_train_cases.NO_GROW) >= 14
    # the live counts: the block edges and both sides of the deck, the benchmark's train, the cap
    for necho in lanes_train_cases.ECHOES:
        name = f"tail_{necho}" if necho in lanes_train_cases.SHORT else f"mse_9x8_{necho}"
        assert kernels(sides["default"][1][name])[0][0] == necho + 1, name
    # the bodies: the excitation and the lone shift run the head cell, which the trace counts as generic
    for name in ("mse_9x8_20", "odd_lead_20", "odd_lead_tail_10", "two_heads_16", "exc_b1_5x4x4_17"):
        assert sides["default"][1][name].rstrip().endswith("body generic+echo-x/4") or ", body generic+echo-x/4\n" in sides["default"][1][name], name
    assert "rows_grow_kernel<2>" in sides["default"][1]["exc_b1_5x4x4_17"] and "rows_grow_kernel<2>" in sides["default"][1]["mse_5x4x4_17"]
