#!/usr/bin/env python3
"""Generate tests/golden/g20_imaging.npz from the reference: spatial read-out of state matrices (DFT / Imaging probes, System).

Run ONLY in the build container, where the upstream reference (py-baudin/epgpy) is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_imaging.py

The reference is imported as a black box and driven through its public API; only the records it returns are written.  The
sequences are defined in tests/imaging_cases.py (`cases`), which the tests call with the device library's operators.

Contents (G20), per case `<case>_<i>`: the record of probe i (`probe=` list of the case, else the probes of the sequence
stacked as simulate returns them), and for two cases the reference's final F / k arrays for the host functions
(`<case>_F`, `<case>_k`).  The weighted 2-D records are zero outside the phantom, which keeps the file small.
"""
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def save_npz(path, arrays):
    """an .npz that np.load reads, with fixed member dates: running the generator again reproduces the file bit for bit"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, arr in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as fid:
                np.lib.format.write_array(fid, np.asanyarray(arr), allow_pickle=False)


def records(simulate, seq, kw):
    out = simulate(seq, **kw)
    return [np.asarray(r) for r in out] if "probe" in kw else [np.asarray(out)]


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.environ.get("EPGPY_REFERENCE", "/root/reference"))
    if not hasattr(np, "asfarray"):      # (NumPy 2 removed it; the reference still calls it)
        np.asfarray = lambda a: np.asarray(a, dtype=np.float64)
    import imaging_cases  # noqa: E402
    from epgpy import operators, functions  # noqa: E402  (the reference)

    ns = types.SimpleNamespace(T=operators.T, E=operators.E, S=operators.S, ADC=operators.ADC, DFT=operators.DFT,
                               Imaging=operators.Imaging, System=operators.System)
    out = {}
    for name, (seq, kw) in imaging_cases.cases(ns).items():
        for key, rec in zip(imaging_cases.record_names(name, kw), records(functions.simulate, seq, kw)):
            out[key] = rec
            print(key, rec.shape, flush=True)
    # final state matrices for the host functions: F and k as the reference's probes see them
    for name in ("dft_1d", "classes_3d"):
        seq, kw = imaging_cases.cases(ns)[name]
        kw = {k: v for k, v in kw.items() if k != "probe"}
        F, k = functions.simulate(seq, probe=["F", "k"], **kw)
        out[name + "_F"], out[name + "_k"] = np.asarray(F)[-1], np.asarray(k)[-1]
        print(name, "F", out[name + "_F"].shape, "k", out[name + "_k"].shape, flush=True)
    path = os.path.join(HERE, "g20_imaging.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
