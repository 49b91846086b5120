"""Sequences for the one-voxel-per-lane variant of the growing launch (rows_grow_lanes_kernel, epgx_grow_lanes_kernels.hip.h;
EPGX_LANES: 0 never, 1 from a threshold of voxels on, 2 whenever the record list is eligible): run as a script it writes their
signals to an .npz -- tests/test_gpu_lanes.py runs it in one child process with EPGX_LANES=0 and in one with EPGX_LANES=2 (the
library reads the variable once per process, at its first launch, so the test's own process cannot choose) and compares.

cases() -> {name: (oracle tuples, product operators, simulate() options, variant the launch must trace under EPGX_LANES=2)}"""
import sys

import numpy as np

ECHOES = (1, 2, 7, 8, 10, 11, 15, 16, 20, 23)      # both sides of the rows ranges' cuts and of the register deck; 23: L = 24


def grids():
    """9 x 8 = 72 voxels (a full wave and one of 8 lanes), 5 x 4 x 4 with a B1 axis (two index spaces), 1 x 3"""
    return {
        "9x8": (np.linspace(200, 3000, 9)[:, None], np.linspace(20, 300, 8)[None, :], 1.0),
        "5x4x4": (np.linspace(200, 3000, 5)[:, None, None], np.linspace(20, 300, 4)[None, :, None],
                  np.linspace(0.8, 1.2, 4)[None, None, :]),
        "1x3": (np.linspace(300, 2500, 1)[:, None], np.linspace(30, 250, 3)[None, :], 1.0),
    }


def cases(epg):
    from tests import reach_cases, sequences as sq
    from oracle import workloads as ow

    out = {}

    def add(name, tuples, variant, **kw):
        made = {}       # a tuple that a description repeats becomes ONE operator object, repeated (as reach_cases)
        for t in tuples:
            if id(t) not in made:
                made[id(t)] = sq.to_ops(epg, [t])[0]
        out[name] = (tuples, [made[id(t)] for t in tuples], kw, variant)

    echo = reach_cases.echo
    exc = [("T", 90, 90)]
    for gname, (T1, T2, B1) in grids().items():
        for necho in ECHOES:
            add(f"mse_{gname}_{necho}", ow.mse_tuples(T1, T2, B1=B1, necho=necho), "lanes", max_nstate=63)
    T1, T2, _ = grids()["9x8"]
    add("unprobed_tail", exc + echo(T1, T2) * 9 + echo(T1, T2, adc=None) * 10, "lanes", max_nstate=63)
    add("every_other_echo", exc + (echo(T1, T2, adc=None) + echo(T1, T2)) * 10, "lanes", max_nstate=63)
    for necho in (9, 20):
        add(f"unfused_{necho}", ow.mse_tuples(T1, T2, necho=necho), "lanes", max_nstate=63, fuse=False)      # pair records
    B1 = np.linspace(0.8, 1.2, 3)[None, None, :]
    alpha, TR = sq.mrf_trains(70)
    add("mrf_40", ow.mrf_tuples(T1[:, :, None], T2[:, :, None], B1, alpha[:40], TR[:40]), "lanes", max_nstate=63)   # folded run
    # one case per reason a list is refused for: each must run the rows variant, and still agree
    add("shift_back", exc + echo(T1, T2) * 10 + echo(T1, T2, shift=-1) * 4 + echo(T1, T2) * 6, "rows", max_nstate=63)
    add("spoiled", exc + echo(T1, T2) * 9 + [("SPOILER",)] + exc + echo(T1, T2) * 11, "rows", max_nstate=63)
    add("max_nstate_10", ow.mse_tuples(T1, T2, necho=20), "rows", max_nstate=10)
    add("mse_31", ow.mse_tuples(T1, T2, necho=31), "rows", max_nstate=63)
    return out


def run_all(epg):
    import os

    only = os.environ.get("EPGX_LANES_CASES")                       # (the test of the default knob runs one case)
    res = {}
    for name, (_, seq, kw, _) in cases(epg).items():
        if only and name not in only.split(","):
            continue
        print(f"[case] {name}", file=sys.stderr, flush=True)       # (with EPGX_TRACE: the library's lines of this case follow)
        res[name] = np.asarray(epg.simulate(seq, **kw))
    return res


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from epgpy_amd import epg

    np.savez(sys.argv[1], **run_all(epg))
