#!/usr/bin/env python3
"""Generate tests/golden/g23_tiled_jacobian.npz from the reference: the Jacobian of a train whose state matrix grows past
1024 orders (the reference puts no limit on derivative states either, epgpy/diff.py:119-139), for the tiled derivative path
of the device library.

Run ONLY in the build container, where the upstream reference (py-baudin/epgpy) is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tiled_jacobian.py

As make_golden_long.py: the reference is imported as a black box and driven through its public API; only the resulting data
(inputs and expected output) are written.  The module itself does not import the reference:
tests/test_gpu_tiled_jacobian.py builds the same train from `inputs` and `sequence` with the device library's operators.

Case (G23), three voxels: a 530-echo CPMG (1060 orders) with refocusing pulses of 140 degrees,
Jacobian(["magnitude", "T2", "alpha"]).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
VARIABLES = ["magnitude", "T2", "alpha"]


def inputs():
    return {"T1": np.array([900.0, 1400.0, 2000.0]), "T2": np.array([220.0, 300.0, 420.0]), "esp": np.array(1.0),
            "alpha": np.array(140.0), "necho": np.array(530)}


def sequence(ops, g):
    """the train built from the operators of `ops` (an object with T, E, S, ADC) and the inputs `g`"""
    T, E, S, ADC = ops.T, ops.E, ops.S, ops.ADC
    e = E(float(g["esp"]) / 2, g["T1"], g["T2"], order1=True)
    rfc = T(float(g["alpha"]), 0, order1=True)
    return [T(90, 90)] + [e, S(1), rfc, S(1), e, ADC] * int(g["necho"])


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.environ.get("EPGPY_REFERENCE", "/root/reference"))
    if not hasattr(np, "asfarray"):      # (NumPy 2 removed it; the reference's spline helper still calls it)
        np.asfarray = lambda a: np.asarray(a, dtype=np.float64)
    from epgpy import operators, functions, diff  # noqa: E402  (the reference)

    g = inputs()
    out = dict(g)
    out["jacobian"] = np.asarray(functions.simulate(sequence(operators, g), probe=diff.Jacobian(VARIABLES)))
    print("jacobian", out["jacobian"].shape, flush=True)
    path = os.path.join(HERE, "g23_tiled_jacobian.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
