"""Jacobians beyond 1024 orders on the tiled path (csrc/epgx_tiled.hip tiled_deriv_kernel): one JSON line per leg.

The 3000-TR unbounded FISP-MRF train of tools/bench_tiled.py over --nvox voxels (default 16 384), differentiated with respect
to one variable (T2) and to as many as one launch carries (_lib.TILED_DERIV_V: T1 and T2).  Next to each: the plain tiled run
of the same sequence in the same process, and the ratio of the two.  The model the ratio is read against is (1 + V) x the
plain path's HBM traffic: every block re-reads and re-writes 1 + V windows instead of one.

    python tools/bench_tiled_jacobian.py [--nvox N] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epgpy_amd import epg, _lib, functions  # noqa: E402


def timed(ctx, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(steps):
        fn()
    return ctx.timer_stop() / steps


def mrf_train(ntr, T1, T2):
    flips = 10 + 60 * np.abs(np.sin(np.arange(ntr) * np.pi / 500))
    rl = {"T1": {"T1": 1}, "T2": {"T2": 1}}
    seq = [epg.T(180, 0), epg.E(20, T1, T2, order1=rl), epg.SPOILER]
    e_te, e_rest = epg.E(2, T1, T2, order1=rl), epg.E(8, T1, T2, order1=rl)
    for i, fa in enumerate(flips):
        seq += [epg.T(float(fa), 90.0 if i % 2 else 0.0), e_te, epg.ADC, e_rest, epg.S(1)]
    return seq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvox", type=int, default=16384)
    ap.add_argument("--ntr", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    ctx = _lib.get_context(None)
    side = int(round(args.nvox ** 0.5))
    T1, T2 = np.linspace(200, 3000, side)[:, None], np.linspace(20, 300, args.nvox // side)[None, :]
    seq = mrf_train(args.ntr, T1, T2)

    enc, _, _ = functions.compile_sequence(seq)
    Kbuf, nv = enc.tiled_capacity(), enc.nvox
    plan = enc.device_plan(ctx)
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nv)
    plain_ms = timed(ctx, lambda: _lib.run_tiled(ctx, plan, 0, nv, None, Kbuf, sig.ptr.value, nv, 0), args.steps, args.warmup)
    plain_names = _lib.tiled_info(ctx, plan, Kbuf)["names"]
    sig.free()

    for variables in (["T2"], ["T1", "T2"][:_lib.TILED_DERIV_V]):
        enc, _, _ = functions.compile_sequence(seq, [epg.Jacobian(["magnitude"] + variables)], variables=variables)
        plan = enc.device_plan(ctx)
        sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nv)
        info = _lib.tiled_deriv_info(ctx, plan, Kbuf)
        ms = timed(ctx, lambda: _lib.run_tiled_deriv(ctx, plan, 0, nv, None, Kbuf, sig.ptr.value, nv, 0), args.steps, args.warmup)
        sig.free()
        V = len(variables)
        print(json.dumps({"leg": f"mrf{args.ntr}_jacobian", "variables": variables, "nvox": nv, "Kbuf": Kbuf, "kernels": info["names"],
                          "launches": info["blocks"] + info["shifts"], "tile_launches": info["tile_launches"],
                          "deriv_ms": round(ms, 3), "plain_kernels": plain_names, "plain_ms": round(plain_ms, 3),
                          "deriv_over_plain": round(ms / plain_ms, 3), "hbm_model": 1 + V}), flush=True)


if __name__ == "__main__":
    main()
