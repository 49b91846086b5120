#!/usr/bin/env python3
"""Generate tests/golden/g18_long_trains.npz from the reference: trains whose state matrix grows past 2048 orders (the
reference's unbounded growth, epgpy/shift.py:86,98), for the tiled path of the device library.

Run ONLY in the build container, where the upstream reference (py-baudin/epgpy) is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_long.py

As make_golden.py: the reference is imported as a black box and driven through its public API; only the resulting data
(inputs and expected outputs) are written.  The module itself does not import the reference: tests/test_gpu_tiled.py builds
the same trains from `inputs` and `sequences` with the device library's operators and compares with the stored signals.

Cases (G18), two voxels each:
  cpmg    an unbounded 1100-echo CPMG train (2200 orders), two T2
  mrf     a 2600-TR FISP-MRF train with a varying flip schedule (2600 orders), two (T1, T2)
  hyper   the hyper-echo of test/test_core.py:9-32 with 2 x 700 pulses (2802 orders), two flip angles
  capped  a mixed-shift train (S(2), S(-1), one S(300)) with S(nmax=2100), Z0 probes included, two T2
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def inputs():
    """the parameters of the four trains (smooth deterministic schedules: the fixture stores only the small ones)"""
    ntr, nrep = 2600, 1500
    i, j = np.arange(ntr), np.arange(nrep)
    return {
        "cpmg_T2": np.array([45.0, 180.0]), "cpmg_esp": np.array(5.0), "cpmg_necho": np.array(1100),
        "mrf_T1": np.array([600.0, 1400.0]), "mrf_T2": np.array([50.0, 150.0]),
        "mrf_flips": 8 + 55 * np.abs(np.sin(i * np.pi / 400)) + 2 * np.sin(i * 0.37) ** 2,
        "hyper_alpha": np.array([10.0, 25.0]), "hyper_npulse": np.array(700),
        "capped_T2": np.array([60.0, 240.0]), "capped_alpha": 95 + 75 * np.sin(j * 1.7), "capped_phi": 90 * np.sin(j * 0.9),
        "capped_nmax": np.array(2100),
    }


def sequences(ops, g):
    """the four trains built from the operators of `ops` (an object with T, E, S, ADC, Adc) and the inputs `g`"""
    T, E, S, ADC = ops.T, ops.E, ops.S, ops.ADC
    half = float(g["cpmg_esp"]) / 2
    e = E(half, 1000.0, g["cpmg_T2"])
    cpmg = [T(90, 90)] + [e, S(1), T(180, 0), S(1), e, ADC] * int(g["cpmg_necho"])
    e_te, e_rest = E(3.0, g["mrf_T1"], g["mrf_T2"]), E(9.0, g["mrf_T1"], g["mrf_T2"])
    mrf = [T(180, 0), E(15.0, g["mrf_T1"], g["mrf_T2"]), ops.SPOILER]
    for i, fa in enumerate(g["mrf_flips"]):
        mrf += [T(float(fa), 90.0 if i % 2 else 0.0), e_te, ADC, e_rest, S(1)]
    alpha = g["hyper_alpha"]
    echo1 = [S(1), T(alpha, 0), S(1), ADC]
    echo2 = [S(1), T(-alpha, 0), S(1), ADC]
    n = int(g["hyper_npulse"])
    hyper = [T(90, 90)] + echo1 * n + [S(1), T(180, 0), S(1)] + echo2 * n
    nmax = int(g["capped_nmax"])
    e3 = E(3.0, 900.0, g["capped_T2"])
    capped = [T(90, 90)]
    for i, (a, p) in enumerate(zip(g["capped_alpha"], g["capped_phi"])):
        capped += [S(2 if i % 3 else -1, nmax=nmax), T(float(a), float(p)), e3]
        if i % 3 == 0:
            capped += [ADC]
        if i == 400:
            capped += [S(300, nmax=nmax), ops.Adc("Z0"), S(-40, nmax=nmax), ADC]
    capped += [ADC]
    return {"cpmg": cpmg, "mrf": mrf, "hyper": hyper, "capped": capped}


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.environ.get("EPGPY_REFERENCE", "/root/reference"))
    if not hasattr(np, "asfarray"):      # (NumPy 2 removed it; the reference's spline helper still calls it)
        np.asfarray = lambda a: np.asarray(a, dtype=np.float64)
    from epgpy import operators, functions  # noqa: E402  (the reference)

    g = inputs()
    out = {k: v for k, v in g.items() if v.size <= 2}
    for name, seq in sequences(operators, g).items():
        out[name] = np.asarray(functions.simulate(seq))
        print(name, out[name].shape, flush=True)
    path = os.path.join(HERE, "g18_long_trains.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
