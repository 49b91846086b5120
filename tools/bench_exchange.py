"""Two-pool RF-spoiled SPGR with exchange (epg.X) over 262 144 compartment groups at K = 128: ms per launch of the whole
train on the fused kernel (xrun_kernel), on the split path (EPGX_XRUN=0, measured in a child process: the library reads
its knobs once per process), and for the same train with a relaxation E in place of X over 524 288 single-compartment
voxels; plus the largest deviation of sampled groups from a NumPy EPG-X recurrence.  Prints one JSON line.

    python tools/bench_exchange.py [--groups 262144] [--trs 100] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epgpy_amd import epg, exchange, _lib  # noqa: E402
from epgpy_amd import functions as _functions  # noqa: E402


def timed(ctx, enc, K, reps):
    plan = enc.device_plan(ctx, K)
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * enc.nvox)
    run = lambda: _lib.run(ctx, plan, 0, plan.n_ops, 0, enc.nvox, None, None, K, sig.ptr.value, enc.nvox, 0)
    run()
    ctx.synchronize()
    best = []
    for _ in range(reps):
        ctx.timer_start()
        run()
        best.append(ctx.timer_stop())
    return float(np.median(best)), plan, sig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=262144)
    ap.add_argument("--trs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--split-only", action="store_true", help="(child) print the ms of this process's launch only")
    args = ap.parse_args()
    M, ntr = args.groups, args.trs
    rng = np.random.default_rng(0)
    dens = [1.0, 1.0]          # a launch from equilibrium (no start state): density 1 in every voxel
    khi = exchange.exchange_matrix(2e-3)
    T2b = rng.uniform(10, 30, M)
    fa = rng.uniform(5, 30, M)
    x = epg.X(5.0, khi, T1=[[1000.0], [500.0]], T2=[np.full(M, 100.0), T2b])
    seq = [[epg.T([fa], 117.0 * i * (i + 1) / 2), epg.ADC, x, epg.S(1)] for i in range(ntr)]
    enc, _, _ = _functions.compile_sequence(seq, options=dict(max_nstate=100))
    ctx = _lib.get_context(0)
    K = enc.capacity()
    ms_x, plan, sig = timed(ctx, enc, K, args.reps)
    kernel = _lib.kernel_for(ctx, plan, K)
    if args.split_only:
        print(json.dumps(dict(kernel=kernel, ms=ms_x)))
        return
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-only", "--groups", str(M), "--trs", str(ntr),
                            "--reps", str(args.reps)], env=dict(os.environ, EPGX_XRUN="0"), capture_output=True, text=True,
                           check=True)
    split = json.loads(child.stdout.strip().splitlines()[-1])

    # the same train with E in place of X, over as many single-compartment voxels
    e = epg.E(5.0, 1000.0, np.concatenate([np.full(M, 100.0), T2b]))
    fa2 = np.concatenate([fa, fa])
    seq_e = [[epg.T(fa2, 117.0 * i * (i + 1) / 2), epg.ADC, e, epg.S(1)] for i in range(ntr)]
    enc_e, _, _ = _functions.compile_sequence(seq_e, options=dict(max_nstate=100))
    ms_e, plan_e, _ = timed(ctx, enc_e, K, args.reps)

    # sampled groups against the NumPy recurrence (no truncation while ntr < 100)
    from tests.exchange_recurrence import recurrence
    got = sig.download(np.complex128, (enc.n_adc,) + enc.grid)
    idx = rng.choice(M, min(args.sample, M), replace=False)
    xs = epg.X(5.0, khi, T1=[[1000.0], [500.0]], T2=[np.full(len(idx), 100.0), T2b[idx]])
    flat = [op for i in range(ntr) for op in (epg.T([fa[idx]], 117.0 * i * (i + 1) / 2), epg.ADC, xs, epg.S(1))]
    want = recurrence(flat, (2, len(idx)), dens, ntr + 1)
    err = float(np.max(np.abs(got[:, :, idx] - want)))
    print(json.dumps(dict(workload=f"2-pool SPGR, {ntr} TR, {M} groups, K={K}", kernel=kernel, fused_ms=ms_x,
                          split_kernel=split["kernel"], split_ms=split["ms"], split_over_fused=split["ms"] / ms_x,
                          e_only_ms=ms_e, e_only_kernel=_lib.kernel_for(ctx, plan_e, K), fused_over_e=ms_x / ms_e,
                          max_err_vs_numpy=err, sampled_groups=int(len(idx)))))


if __name__ == "__main__":
    main()
