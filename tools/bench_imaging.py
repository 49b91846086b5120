"""Spatial read-out (epg.DFT / epg.Imaging) on the device against the same acquisition on the host, for

  gre   a 2-D gradient-echo acquisition of a synthetic phantom: 64 x 64 pixels x 3 tissues, System(weights=) + Imaging with
        reduce=True, one k-space sample per acquisition (integer shifts, kvalue = 2 pi / FOV)
  dft   65 536 (T1, T2) voxels x 301 positions x 128 orders, DFT, unreduced

Per workload: device time of one epgx_state_dft CALL on the final state matrix (`call_ms`, HIP events around the call: block
allocation, pageable upload of the k / w / position tables with its stream synchronisation, fold kernel, DFT kernel -- NOT the
kernels alone: their times come from `rocprofv3 --kernel-trace --stats` on an --acquire-only run), 8 nvox nrow npos flop over
that time as a share of the fp64 vector peak (`share_of_fp64_peak_of_call`: a lower bound of the kernel's share), the
same acquisition on the host (state download + utils.imaging, what Probe(callable) costs a user without these probes), wall
time of simulate() with the device probes and -- for `gre` -- with host probes.  Appends one JSON line per workload to --out.

    python tools/bench_imaging.py [--workload gre|dft|both] [--pixels 64] [--lines 64] [--voxels 256] [--positions 301]
                                  [--orders 128] [--reps 5] [--host-voxels 4096] [--out profiles/imaging_bench.jsonl]
    python tools/bench_imaging.py --workload dft --acquire-only 20      # 20 acquisitions, nothing else (for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epgpy_amd import epg, utils, probe, _lib  # noqa: E402

FP64_PEAK = 78.6e12          # MI355X vector fp64, flop/s


def gre(args):
    """(operators up to the last acquisition, positions, Imaging options, system weights, kvalue)"""
    n, fov = args.pixels, 0.2
    ax = (np.arange(n) - n // 2) * (fov / n)
    pix = np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2)
    x, y = pix.T / fov
    r = np.hypot(x, y)
    pd = np.stack([np.where(r < 0.17, 1.0, 0.0), np.where((r >= 0.17) & (r < 0.3), 0.6 + 0.4 * x, 0.0),
                   np.where((np.abs(x - 0.33) < 0.07) & (np.abs(y + 0.3) < 0.1), 0.8, 0.0)])
    relax = epg.E(0.1, 1000, [50.0, 70.0, 90.0])

    def sequence(sample):
        seq = [epg.System(weights=pd, kvalue=2 * np.pi / fov)]
        for j in range(args.lines):
            seq += [epg.T(30, 117.0 * j * (j + 1) / 2), epg.S([-(n // 2), j - args.lines // 2])]
            seq += [sample(j), relax, epg.S([1, 0])] * n + [epg.S([n // 4, args.lines // 2 - j])]      # (not rewound: the lines mix)
        return seq
    return sequence, pix, dict(voxel_size=fov / n, reduce=True), pd


def dft(args):
    g = args.voxels
    T1, T2 = np.linspace(300.0, 3000.0, g)[:, None], np.linspace(20.0, 300.0, g)[None, :]
    pos = 1e-2 * np.linspace(-0.5, 0.5, args.positions)
    relax = epg.E(1.0, T1, T2, 0.01)

    def sequence(sample):
        seq = []
        for i in range(args.orders - 1):
            seq += [epg.T(12, 7 * i), relax, epg.S(1)]
        return seq + [sample(0)]
    return sequence, pos, dict(voxel_shape="point", reduce=False), None


def final_state(sequence, kw):
    """the state matrix at the last acquisition of the sequence"""
    held = []
    grab = epg.Probe(lambda sm: (held.append(sm.copy()), 0.0)[1])
    seq = sequence(lambda j: epg.NULL)
    last = max(i for i, op in enumerate(seq) if op is epg.NULL)
    epg.simulate(seq[:last] + [grab], **kw)
    return held[-1]


def measure(name, args):
    sequence, pos, opts, weights = (gre if name == "gre" else dft)(args)
    kw = {} if name == "gre" else {"kvalue": 500.0}
    sm = final_state(sequence, kw)
    ctx = sm._ctx
    flat = np.asarray(pos).reshape(len(pos), -1)
    nvox, nrow, npos, d = sm.size, sm.nstate + 1, len(flat), flat.shape[1]
    k_tab, w_tab, lead = probe.readout_tables(sm._kspace, sm.nstate, sm.kvalue, d, opts.get("voxel_shape", "box"),
                                              opts.get("voxel_size", 1))
    out = _lib.DeviceBuffer(ctx, 16 * nvox * npos)
    acquire = lambda: _lib.state_dft(ctx, sm._state, 0, nvox, k_tab[0], w_tab[0], flat, 1.0, out.ptr.value)     # noqa: E731
    if args.acquire_only:
        for _ in range(args.acquire_only):
            acquire()
        ctx.synchronize()
        return None
    acquire()
    ctx.synchronize()
    device = []
    for _ in range(args.reps):
        ctx.timer_start()
        acquire()
        device.append(ctx.timer_stop())
    flop = 8.0 * nvox * nrow * npos
    res = dict(workload=name, label=args.label, nvox=nvox, nrow=nrow, K=sm._state.K, npos=npos, columns=d, classes=len(k_tab),
               flop=flop, call_ms=float(np.median(device)), call_ms_all=[round(v, 4) for v in device],
               share_of_fp64_peak_of_call=flop / (float(np.median(device)) * 1e-3) / FP64_PEAK)

    # the whole acquisition as the probe does it (tables, launch, reduction, download) and on the host (download + NumPy)
    full = []
    for _ in range(args.reps):
        tic = time.perf_counter()
        got = probe.read_out(sm, pos, weights=weights, **opts)
        full.append((time.perf_counter() - tic) * 1e3)
    hv = min(args.host_voxels or nvox, nvox)
    tic = time.perf_counter()
    F, k = sm.F, sm.k[..., :3]
    download_ms = (time.perf_counter() - tic) * 1e3
    Fh = F.reshape(nvox, -1)[:hv] if hv < nvox else F
    k = k if hv == nvox else k.reshape((1,) + k.shape[-2:])      # (one coordinate set for all voxels in these workloads)
    tic = time.perf_counter()
    want = utils.imaging(pos, Fh, k, weights=weights if hv == nvox else None, **opts)
    host_ms = (time.perf_counter() - tic) * 1e3
    res.update(acquire_ms=float(np.median(full)), acquire_ms_all=[round(v, 3) for v in full], host_download_ms=download_ms,
               host_imaging_ms=host_ms, host_voxels=hv, host_ms_scaled=download_ms + host_ms * nvox / hv)
    if hv == nvox:
        res["max_abs_diff_device_host"] = float(np.max(np.abs(np.asarray(got) - np.asarray(want))))
    else:
        res["max_abs_diff_device_host"] = float(np.max(np.abs(np.asarray(got).reshape(nvox, -1)[:hv] - np.asarray(want).reshape(hv, -1))))

    # simulate(): device probes, and -- where it ends in reasonable time -- the same sequence with host probes
    def wall(seq, reps, warm=True):
        if warm:
            epg.simulate(seq, **kw)
        times = []
        for _ in range(reps):
            tic = time.perf_counter()
            result = epg.simulate(seq, **kw)
            times.append((time.perf_counter() - tic) * 1e3)
        return float(np.median(times)), result
    make = (lambda j: epg.Imaging(pos, **opts)) if name == "gre" else (lambda j: epg.DFT(pos))
    res["simulate_ms"], sig = wall(sequence(make), args.reps)
    res["acquisitions"] = int(np.asarray(sig).shape[0])
    if name == "gre":
        host_probe = lambda j: epg.Probe(lambda sm: utils.imaging(pos, sm.F, sm.k[..., :3], weights=weights, **opts))     # noqa: E731
        res["simulate_host_probes_ms"], ref = wall(sequence(host_probe), 1, warm=False)
        res["max_abs_diff_simulate"] = float(np.max(np.abs(np.asarray(sig) - np.asarray(ref))))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=("gre", "dft", "both"))
    ap.add_argument("--pixels", type=int, default=64)
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--voxels", type=int, default=256, help="dft: the (T1, T2) grid is voxels x voxels")
    ap.add_argument("--positions", type=int, default=301)
    ap.add_argument("--orders", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-voxels", type=int, default=4096, help="dft: voxels of the host acquisition (scaled to all); 0: all")
    ap.add_argument("--acquire-only", type=int, default=0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    for name in (("gre", "dft") if args.workload == "both" else (args.workload,)):
        res = measure(name, args)
        if res is None:
            continue
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
