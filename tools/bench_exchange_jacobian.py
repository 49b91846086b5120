"""The exchange benchmark train of tools/bench_exchange.py (two-pool RF-spoiled SPGR, 100 TR, 262 144 compartment groups,
K = 128) with ONE derivative state through X (dxrun_kernel<2, 2, 1>: the exchange rate), against (a) the plain launch
(xrun_kernel<2, 2, false>) and (b) two plain launches -- what a central finite difference of that variable costs.  All three
in one process.  Prints one JSON line.

    python tools/bench_exchange_jacobian.py [--groups 262144] [--trs 100] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epgpy_amd import epg, exchange, _lib  # noqa: E402
from epgpy_amd import functions as _functions  # noqa: E402
from tools.bench_exchange import timed  # noqa: E402


def train(M, ntr, order1):
    rng = np.random.default_rng(0)
    T2b, fa = rng.uniform(10, 30, M), rng.uniform(5, 30, M)
    x = epg.X(5.0, 2e-3, T1=[[1000.0], [500.0]], T2=[np.full(M, 100.0), T2b], **({"order1": {"k": {"khi": 1}}} if order1 else {}))
    return [[epg.T([fa], 117.0 * i * (i + 1) / 2), epg.ADC, x, epg.S(1)] for i in range(ntr)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=262144)
    ap.add_argument("--trs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ctx = _lib.get_context(0)
    enc, _, _ = _functions.compile_sequence(train(args.groups, args.trs, False), options=dict(max_nstate=100))
    K = enc.capacity()
    ms_plain, plan, _ = timed(ctx, enc, K, args.reps)
    denc, _, _ = _functions.compile_sequence(train(args.groups, args.trs, True), options=dict(max_nstate=100), variables=["k"])
    ms_jac, dplan, _ = timed(ctx, denc, K, args.reps)
    print(json.dumps(dict(workload=f"2-pool SPGR, {args.trs} TR, {args.groups} groups, K={K}, V=1", kernel=_lib.kernel_for(ctx, dplan, K),
                          jacobian_ms=ms_jac, plain_kernel=_lib.kernel_for(ctx, plan, K), plain_ms=ms_plain,
                          jacobian_over_plain=ms_jac / ms_plain, finite_difference_ms=2 * ms_plain,
                          jacobian_over_finite_difference=ms_jac / (2 * ms_plain))))


if __name__ == "__main__":
    main()
