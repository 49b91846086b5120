"""20-echo CPMG with 128-sample shaped refocusing pulses that carry T1 / T2 / off-resonance, over 201 positions x 64 x 64
(T1, T2) voxels, state-resident: wall time per simulate() and kernel time (HIP events) per launch of the train, for

  collapsed   the pulse as ONE EPGX_OP_MAT0 record per echo, its table multiplied up by chain_kernel (this commit's default)
  members     the same RFPulse with simulate(collapse=False): 2 x 128 primitive records per echo
  primitives  the T / E list built by hand, without RFPulse -- the only form a commit without epg.RFPulse can run, so the
              baseline when this file is run there

plus the device time of creating the collapsed plan (upload + assemble + chain_kernel), the chain's executed flop, and the
largest difference between the variants.  Appends one JSON line to --out (default: stdout only).

    python tools/bench_rfpulse.py [--positions 201] [--grid 64] [--samples 128] [--echoes 20] [--reps 5] [--out FILE]
    python tools/bench_rfpulse.py --plan-only 20        # create the collapsed plan 20 times (for a kernel trace of chain_kernel)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epgpy_amd import epg, _lib  # noqa: E402
from epgpy_amd import functions as _functions  # noqa: E402

FP64_PEAK = 78.6e12          # MI355X vector fp64, flop/s
FLOP_MAT, FLOP_E = 113, 29   # per step and table entry (chain_kernel: apply_mat, apply_e)
GAMMA = 42.576e3


def workload(args):
    n = args.samples
    x = np.linspace(-3, 3, n)
    wave = (np.sinc(x) * np.hamming(n)).astype(np.complex128)
    duration = 2.56
    freqs = (8.0 * 1e-6 * GAMMA * 16.0 * np.linspace(-0.5, 0.5, args.positions))[:, None, None]
    T1 = np.linspace(300.0, 3000.0, args.grid)[None, :, None]
    T2 = np.linspace(20.0, 300.0, args.grid)[None, None, :]
    rf = 1.0 / np.abs(wave.sum())          # 180 degrees
    relax = epg.E(3.0, T1, T2)
    variants = {}
    # by hand: one T per sample, ONE relaxation object for all of them (equal durations)
    inner = epg.E(duration / n, T1, T2, freqs)
    hand = [op for v in wave for op in (epg.T(180 * abs(v) * rf, float(np.angle(v, deg=True))), inner)]
    train = lambda rfc: [epg.T(90, 90)] + [relax, epg.S(1), rfc, epg.S(1), relax, epg.ADC] * args.echoes      # noqa: E731
    variants["primitives"] = ([epg.T(90, 90)] + ([relax, epg.S(1)] + hand + [epg.S(1), relax, epg.ADC]) * args.echoes, {})
    if hasattr(epg, "RFPulse"):
        pulse = epg.RFPulse(wave, duration, rf=rf, alpha=180, T1=T1, T2=T2, g=freqs)
        variants["collapsed"] = (train(pulse), {})
        variants["members"] = (train(pulse), {"collapse": False})
    return variants


def measure(seq, kw, reps):
    ctx = _lib.get_context(0)
    enc, _, _ = _functions.compile_sequence(seq, **kw)
    K = enc.capacity(resident=True)
    ctx.synchronize()
    ctx.timer_start()
    plan = enc.device_plan(ctx, K)
    plan_ms = ctx.timer_stop()
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * enc.nvox)
    run = lambda: _lib.run(ctx, plan, 0, plan.n_ops, 0, enc.nvox, None, None, K, sig.ptr.value, enc.nvox, 0)      # noqa: E731
    run()
    ctx.synchronize()
    kernel = []
    for _ in range(reps):
        ctx.timer_start()
        run()
        kernel.append(ctx.timer_stop())
    epg.simulate(seq, **kw)                      # warm: tables, page-locked result blocks
    wall = []
    for _ in range(reps):
        tic = time.perf_counter()
        out = epg.simulate(seq, **kw)
        wall.append((time.perf_counter() - tic) * 1e3)
    arrays = enc.plan_arrays(K)
    res = dict(kernel=_lib.kernel_for(ctx, plan, K), K=K, records=int(len(arrays["ops"])), kernel_ms=float(np.median(kernel)),
               kernel_ms_all=[round(v, 4) for v in kernel], wall_ms=float(np.median(wall)), wall_ms_all=[round(v, 3) for v in wall],
               plan_create_device_ms=plan_ms)
    if arrays.get("chain"):
        entries, flop = 0, 0
        for _, space, steps in arrays["chain"]:
            entries = int(np.prod([g for g, st in zip(enc.grid, enc.spaces[space]) if st])) if space >= 0 else 1
            count = 0
            for st in steps:
                count = int(st["count"]) or count
                flop += entries * count * (FLOP_E if st["kind"] == _lib.OP_E else FLOP_MAT)
        res.update(chain_entries=entries, chain_steps=int(sum(len(s) for _, _, s in arrays["chain"])), chain_flop=int(flop),
                   chain_ms_at_fp64_peak=flop / FP64_PEAK * 1e3)
    return res, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=201)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--echoes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--plan-only", type=int, default=0)
    args = ap.parse_args()
    variants = workload(args)
    if args.plan_only:
        seq, kw = variants["collapsed"]
        ctx = _lib.get_context(0)
        enc, _, _ = _functions.compile_sequence(seq, **kw)
        for _ in range(args.plan_only):
            enc.device_plan(ctx, enc.capacity(resident=True))
        ctx.synchronize()
        return
    result = dict(label=args.label, workload=f"{args.echoes}-echo CPMG, {args.samples}-sample pulses, "
                                             f"{args.positions} x {args.grid} x {args.grid} voxels", has_rfpulse=hasattr(epg, "RFPulse"))
    outs = {}
    for name, (seq, kw) in variants.items():
        result[name], outs[name] = measure(seq, kw, args.reps)
    base = outs["primitives"]
    for name, out in outs.items():
        if name != "primitives":
            result[name]["max_abs_diff_to_primitives"] = float(np.max(np.abs(out - base)))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
