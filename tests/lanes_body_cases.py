"""Sequences for the record bodies of the one-voxel-per-lane variant (rows_grow_lanes_kernel: the generic per-cell body and the
specialised bodies that run the cells in blocks, epgx_lanes_bodies.h; EPGX_LANES_BODY=0 runs the generic body everywhere):
the cases of tests/lanes_cases.py and, on its 9 x 8 grid (a full wave and a wave of 8 lanes), the trains that put the window's
top on both sides of every block boundary and of the register deck.  Run as a script it writes the signals to an .npz, like
tests/lanes_cases.py -- tests/test_gpu_lanes_bodies.py runs it in two child processes and compares.

cases() -> {name: (oracle tuples, product operators, simulate() options, variant, bodies the launch must trace by default)}

An n-echo train opens the windows 0 .. lim with lim = 1, 3, 5 ... up to n and down again: L = n + 1 live orders at most.
With blocks of B = 4 cells and a deck of D = 14 (15 fits the registers as well and is covered) the edges are the n with
n + 1 in {B, B + 1, 2 B, 2 B + 1, D - 1, D, D + 1, D + 2}.  A train's lim is odd, so its partial top block holds 2 or 4
cells; a lone S(+1) behind the excitation makes the rising half even: lengths 3 and 1."""
import sys

import numpy as np

BLOCK, DECKS = 4, (14, 15)
EDGES = sorted({n1 - 1 for n1 in (BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1)} |
               {d + k - 1 for d in DECKS for k in (-1, 0, 1, 2)})          # 3, 4, 7, 8, 12 .. 16
ECHO = "generic+echo-x/4"       # the excitation has no body of its own, the folded echo has
GENERIC = "generic"


def shipped_body(name):
    """what the launches of tests/lanes_cases.py trace: unfused pairs and folded MRF records have no specialised body"""
    return GENERIC if name.startswith(("unfused_", "mrf_")) else ECHO


def cases(epg):
    from tests import lanes_cases, reach_cases, sequences as sq
    from oracle import workloads as ow

    out = {name: c + (shipped_body(name),) for name, c in lanes_cases.cases(epg).items()}

    def add(name, tuples, variant, body, **kw):
        if name in out:         # (an edge the shipped cases already hold)
            return
        made = {}
        for t in tuples:
            if id(t) not in made:
                made[id(t)] = sq.to_ops(epg, [t])[0]
        out[name] = (tuples, [made[id(t)] for t in tuples], kw, variant, body)

    T1, T2, _ = lanes_cases.grids()["9x8"]
    for necho in EDGES:
        add(f"mse_9x8_{necho}", ow.mse_tuples(T1, T2, necho=necho), "lanes", ECHO, max_nstate=63)
    exc, echo = [("T", 90, 90)], reach_cases.echo
    for necho in (10, 20):      # top partial blocks of 3 and 1 cells on the way up, 4 and 2 on the way down; 20: through the deck
        add(f"odd_lead_{necho}", exc + [("S", 1)] + echo(T1, T2) * necho, "lanes", ECHO, max_nstate=63)
    add("unfused_13", ow.mse_tuples(T1, T2, necho=13), "lanes", GENERIC, max_nstate=63, fuse=False)
    return out


def run_all(epg):
    res = {}
    for name, (_, seq, kw, _, _) in cases(epg).items():
        print(f"[case] {name}", file=sys.stderr, flush=True)       # (with EPGX_TRACE: the library's lines of this case follow)
        res[name] = np.asarray(epg.simulate(seq, **kw))
    return res


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from epgpy_amd import epg

    np.savez(sys.argv[1], **run_all(epg))
