"""Sequences for the ranges of rows_grow_kernel that run at the orders which can still reach a probe (grow_reach, epgx_planner.cpp):
run as a script it writes their signals to an .npz -- tests/test_gpu_reach.py runs it in a child process with EPGX_REACH=0
(the library reads the variable once per process) and compares with its own results.

cases() -> {name: (oracle tuples or None, product operators, simulate() options)}"""
import sys

import numpy as np


def echo(T1, T2, adc=("ADC",), shift=1, FA=120.0, ESP=10.0):
    return [("S", shift), ("E", ESP / 2, T1, T2, 0), ("T", FA, 0), ("S", shift), ("E", ESP / 2, T1, T2, 0)] + ([adc] if adc else [])


def cases(epg):
    from tests import grow_cases, sequences as sq
    from oracle import workloads as ow

    out = {}
    for name, (seq, kw) in grow_cases.cases(epg).items():
        out["grow_" + name] = (None, seq, kw)

    def add(name, tuples, **kw):
        # a tuple that a description repeats becomes ONE operator object, repeated: what the run-length folding of the record
        # list -- and with it the growing kernel -- is taken for (workloads.mse_sequence builds its trains the same way)
        made = {}
        for t in tuples:
            if id(t) not in made:
                made[id(t)] = sq.to_ops(epg, [t])[0]
        out[name] = (tuples, [made[id(t)] for t in tuples], kw)

    T1 = np.linspace(200, 3000, 7)[:, None]
    T2 = np.linspace(20, 300, 5)[None, :]                        # 35 voxels: the last wavefront holds 3
    for necho in range(1, 41):                                   # every combination of capacities: no narrowing possible
        for nmax in (63, 10, 20):                                # (short trains), narrowing right behind the widening (9 .. 15 echoes), ...
            add(f"mse_{necho}_n{nmax}", ow.mse_tuples(T1, T2, necho=necho), max_nstate=nmax)
    exc = [("T", 90, 90)]
    add("unprobed_tail", exc + echo(T1, T2) * 6 + echo(T1, T2, adc=None) * 30, max_nstate=63)
    add("unprobed_tail_long_head", exc + echo(T1, T2) * 18 + echo(T1, T2, adc=None) * 12, max_nstate=63)
    for necho in (5, 12, 20, 36):
        add(f"single_adc_{necho}", exc + echo(T1, T2, adc=None) * (necho - 1) + echo(T1, T2), max_nstate=63)
    add("z0_probes", exc + echo(T1, T2, adc=("ADC", "Z0")) * 20, max_nstate=63)
    add("f0_and_z0", exc + (echo(T1, T2) + [("ADC", "Z0")]) * 24, max_nstate=63)
    add("shift_back", exc + echo(T1, T2) * 10 + echo(T1, T2, shift=-1) * 4 + echo(T1, T2) * 9, max_nstate=63)
    add("spoiled", exc + echo(T1, T2) * 9 + [("SPOILER",)] + exc + echo(T1, T2) * 11, max_nstate=63)
    add("reset", exc + echo(T1, T2) * 12 + [("RESET",)] + exc + echo(T1, T2) * 10, max_nstate=63)
    add("reset_in_tail", exc + echo(T1, T2) * 18 + [("RESET",)] + exc + echo(T1, T2) * 3, max_nstate=63)
    for necho in (9, 12, 20, 27):
        add(f"unfused_{necho}", ow.mse_tuples(T1, T2, necho=necho), max_nstate=63, fuse=False)      # the pair runs
    B1 = np.linspace(0.8, 1.2, 3)[None, None, :]
    alpha, TR = sq.mrf_trains(70)
    for ntr in (24, 40, 70):                                     # folded single runs, one shift per repetition
        add(f"mrf_{ntr}", ow.mrf_tuples(T1[:, :, None], T2[:, :, None], B1, alpha[:ntr], TR[:ntr]), max_nstate=63)
    for n1, n2 in ((1, 1), (1, 3), (3, 6), (1, 17), (13, 5)):    # 1, 3, 18, 17, 65 voxels: the tail groups
        t1, t2 = np.linspace(300, 2500, n1)[:, None], np.linspace(30, 250, n2)[None, :]
        add(f"grid_{n1}x{n2}", ow.mse_tuples(t1, t2, necho=20), max_nstate=63)
        add(f"grid_{n1}x{n2}_12", ow.mse_tuples(t1, t2, necho=12), max_nstate=63)
    return out


def run_all(epg):
    res = {}
    for name, (_, seq, kw) in cases(epg).items():
        res[name] = np.asarray(epg.simulate(seq, **kw))
    return res


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from epgpy_amd import epg

    np.savez(sys.argv[1], **run_all(epg))
