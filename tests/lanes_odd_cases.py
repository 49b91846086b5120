"""Sequences for rows_grow_lanes_kernel_odd (epgx_grow_lanes_odd_kernels.hip.h): the cases of tests/lanes_train_cases.py as they
stand -- 9 x 8 voxels (a full wave and a wave of 8 lanes), 5 x 4 x 4 with two index spaces, echo counts at the block edges and
up to the cap, the tail_<n> windows, lists that are no trains or have a shifting head record -- plus the probe patterns
they lack, at 9 x 8: an unprobed tail behind 9 probed echoes, a probe behind every other echo (which the planner does not turn
into a growing launch: it stays for the agreement), and unprobed echoes BETWEEN probed ones (5 probed, 5 unprobed, 10 probed:
executions whose cells run with no probe behind them, the state carried across them to the probes that follow).  Run as a script it
writes the signals to an .npz; tests/test_gpu_lanes_odd.py runs it in two child processes and compares.

cases() -> {name: (oracle tuples, product operators, simulate() options, kernel the launch traces WITHOUT the odd kernel)}
is_odd(case) -> whether the list is LanesPlan::odd, from the operators alone: a train whose shifts up to the last probe are an
even number (a lone S(+1) behind the excitation makes them odd; every echo adds two)."""
import sys

import numpy as np


def cases(epg):
    from tests import lanes_cases, lanes_train_cases, reach_cases, sequences as sq

    out = dict(lanes_train_cases.cases(epg))
    T1, T2, _ = lanes_cases.grids()["9x8"]
    exc, echo = [("T", 90, 90)], reach_cases.echo
    extra = {"unprobed_tail_9": exc + echo(T1, T2) * 9 + echo(T1, T2, adc=None) * 10,
             "every_other_echo_20": exc + (echo(T1, T2, adc=None) + echo(T1, T2)) * 10,
             "unprobed_middle_20": exc + echo(T1, T2) * 5 + echo(T1, T2, adc=None) * 5 + echo(T1, T2) * 10}
    for name, tuples in extra.items():
        made = {}
        for t in tuples:
            if id(t) not in made:
                made[id(t)] = sq.to_ops(epg, [t])[0]
        out[name] = (tuples, [made[id(t)] for t in tuples], {"max_nstate": 63}, lanes_train_cases.TRAIN)
    return out


def is_odd(case):
    from tests import lanes_train_cases

    tuples, _, _, kernel = case
    last = max(i for i, t in enumerate(tuples) if t[0] == "ADC")
    shifts = sum(1 for t in tuples[:last] if t[0] == "S")
    return kernel == lanes_train_cases.TRAIN and shifts % 2 == 0


def run_all(epg):
    res = {}
    for name, (_, seq, kw, _) in cases(epg).items():
        print(f"[case] {name}", file=sys.stderr, flush=True)       # (with EPGX_TRACE: the library's lines of this case follow)
        res[name] = np.asarray(epg.simulate(seq, **kw))
    return res


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from epgpy_amd import epg

    np.savez(sys.argv[1], **run_all(epg))
