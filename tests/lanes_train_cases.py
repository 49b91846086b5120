"""Sequences for the two kernels of the one-voxel-per-lane variant (epgx_grow_lanes_kernels.hip.h): a TRAIN -- head records before
the first shift, then only records with a specialised body (LanesPlan::train) -- runs rows_grow_lanes_kernel<NSP, true>, which
has no generic body and a register deck of DECK = 16 orders; every other eligible list, and every list under EPGX_LANES_TRAIN=0 or
EPGX_LANES_BODY=0, runs rows_grow_lanes_kernel<NSP, false> (deck 14).  Run as a script it writes the signals to an .npz, like
tests/lanes_body_cases.py -- tests/test_gpu_lanes_train.py runs it in four child processes and compares.

cases() -> {name: (oracle tuples, product operators, simulate() options, kernel the launch must trace by default)}

On the 9 x 8 grid (a full wave and a wave of 8 lanes) an n-echo train opens the windows 0 .. lim, lim = 1, 3 ... n and down
again, L = n + 1 live orders: n + 1 in {DECK - 1 .. DECK + 2} puts the top of the window on both sides of the deck (the first
LDS slot, the last register slot), n = 3, 4, 7, 8 on both sides of the edges of blocks of four cells, n = 20 is the benchmark's
train and n = 23 the cap L = 24.  A train of up to 15 echoes stays within 32 orders and never becomes a growing launch at 64:
the `tail_<n>` cases put TAIL unprobed echoes behind n probed ones -- the launch then grows, and its window is that of the n
probed echoes, L = n + 1 (the shifts behind the last probe do not count), so the edges below the deck reach the kernel as well."""
import sys

import numpy as np

DECK, BLOCK = 16, 4
ECHOES = sorted({DECK + k - 1 for k in (-1, 0, 1, 2)} | {3, 4, 7, 8} | {20, 23})
SHORT = (3, 4, 7, 8, DECK - 2, DECK - 1)         # mse_9x8_<n> without a growing launch; tail_<n> stands in for them
TAIL = 14
NO_GROW = tuple(f"mse_9x8_{n}" for n in SHORT) + ("odd_lead_10",)       # (21 shifts: 22 orders; odd_lead_tail_10 stands in)
TRAIN, ANY = "train", "any list"        # the kernel names of the `variant lanes` trace line


def cases(epg):
    from tests import lanes_cases, reach_cases, sequences as sq
    from oracle import workloads as ow

    out = {}

    def add(name, tuples, kernel, **kw):
        made = {}
        for t in tuples:
            if id(t) not in made:
                made[id(t)] = sq.to_ops(epg, [t])[0]
        out[name] = (tuples, [made[id(t)] for t in tuples], kw, kernel)

    grids = lanes_cases.grids()
    T1, T2, _ = grids["9x8"]
    for necho in ECHOES:
        add(f"mse_9x8_{necho}", ow.mse_tuples(T1, T2, necho=necho), TRAIN, max_nstate=63)
    exc, echo = [("T", 90, 90)], reach_cases.echo
    for necho in SHORT:
        add(f"tail_{necho}", exc + echo(T1, T2) * necho + echo(T1, T2, adc=None) * TAIL, TRAIN, max_nstate=63)
    for necho in (10, 20):      # a lone S(+1) behind the excitation: a head record with a trailing shift, even windows on the way up
        add(f"odd_lead_{necho}", exc + [("S", 1)] + echo(T1, T2) * necho, TRAIN, max_nstate=63)
    add("odd_lead_tail_10", exc + [("S", 1)] + echo(T1, T2) * 10 + echo(T1, T2, adc=None) * TAIL, TRAIN, max_nstate=63)
    # two records before the first shift: a relaxation with precession between two rotations keeps them apart
    add("two_heads_16", exc + [("E", 3.0, T1, T2, 0.1), ("T", 15, 40)] + echo(T1, T2) * 16, TRAIN, max_nstate=63)
    T1, T2, B1 = grids["5x4x4"]
    # two index spaces: only the excitation depends on B1, the echoes fuse on the host as they do on the 9 x 8 grid
    add("exc_b1_5x4x4_17", [("T", 90 * B1, 90)] + echo(T1, T2) * 17, TRAIN, max_nstate=63)
    # with B1 in the refocusing pulse as well the relaxations fold at run time and the first shift closes the excitation's record:
    # the first echo is then a record of its own shape (no leading shift), which has no body -- not a train
    add("mse_5x4x4_17", ow.mse_tuples(T1, T2, B1=B1, necho=17), ANY, max_nstate=63)
    # lists that are no trains keep the kernel with the generic body
    T1, T2, _ = grids["9x8"]
    add("unfused_17", ow.mse_tuples(T1, T2, necho=17), ANY, max_nstate=63, fuse=False)
    B1 = np.linspace(0.8, 1.2, 3)[None, None, :]
    alpha, TR = sq.mrf_trains(70)
    add("mrf_40", ow.mrf_tuples(T1[:, :, None], T2[:, :, None], B1, alpha[:40], TR[:40]), ANY, max_nstate=63)
    return out


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
