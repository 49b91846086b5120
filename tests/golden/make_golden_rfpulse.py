#!/usr/bin/env python3
"""Generate tests/golden/g19_rfpulse.npz from the reference: shaped RF pulses (epgpy/rfpulse.py) and slice profiles.

Run ONLY in the build container, where the upstream reference (py-baudin/epgpy) is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rfpulse.py

As make_golden_long.py: the reference is imported as a black box and driven through its public API; only the resulting data
(inputs and expected outputs) are written.  The module itself does not import the reference: the tests build the same pulses
and sequences from `waveforms`, `host_values` and `cases` with the device library's operators and compare with the stored arrays.

Contents (G19):
  wave_*            the waveforms: a Hamming-windowed sinc (64 samples), a quadratic-phase sinc (128 samples: its phase varies,
                    so estimate_rf goes through the optimiser), a hard pulse (1 sample)
  rf_*, alpha_*     estimate_rf / estimate_alpha values
  positions, freqs, back     spatial_range, space_to_freq, freq_to_space
  <case>_F0, <case>_Z0       simulate outputs of `cases`
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

GRADIENT, FOV, NPOINT = 10.0, 20.0, 41      # mT/m, mm, positions


def waveforms():
    x64 = np.linspace(-3, 3, 64)
    x128 = np.linspace(-4, 4, 128)
    return {
        "sinc64": (np.sinc(x64) * np.hamming(64)).astype(np.complex128),
        "quad128": np.sinc(x128) * np.hamming(128) * np.exp(1j * 1.5 * x128 ** 2),
        "hard": np.array([1.0 + 0j]),
    }


def host_values(ns):
    """the host functions of the namespace `ns` (estimate_rf, estimate_alpha, spatial_range, space_to_freq, freq_to_space)"""
    w = waveforms()
    out = {}
    for name, wave in w.items():
        for alpha in (90, 180):
            out[f"rf_{name}_{alpha}"] = np.asarray(ns.estimate_rf(wave, alpha))
        out[f"alpha_{name}"] = np.asarray([ns.estimate_alpha(wave, rf) for rf in (0.1, 0.37, 1.3)])
    out["positions"] = ns.spatial_range(FOV, NPOINT)
    out["freqs"] = ns.space_to_freq(GRADIENT, out["positions"])
    out["back"] = ns.freq_to_space(GRADIENT, out["freqs"])
    return out


PREPARED = np.array([[0.05 + 0.02j, 0.2 - 0.1j, 0.03 - 0.04j],
                     [0.3 + 0.1j, 0.3 - 0.1j, 0.6],
                     [0.2 + 0.1j, 0.05 - 0.02j, 0.03 + 0.04j]])      # orders -1, 0, +1 of a state matrix with the EPG symmetry


def cases(ns):
    """{name: (sequence, simulate keywords)} built from the namespace `ns` (RFPulse, encode_phase, T, E, S, ADC)"""
    w = waveforms()
    out = {}
    for alpha in (90, 180):
        pulse = ns.RFPulse(w["sinc64"], 2.0, alpha=alpha)
        profile = ns.encode_phase(pulse, GRADIENT, FOV, npoint=NPOINT, rewind=True)
        out[f"profile{alpha}_eq"] = ([profile, ns.ADC], {})
        out[f"profile{alpha}_prep"] = ([profile, ns.ADC], {"init": PREPARED})
    # relaxation and off-resonance arrays inside the pulse: (T2 x g) grid
    T2 = np.array([20.0, 60.0, 200.0])
    g = np.linspace(-1.5, 1.5, 7)[None, :]
    out["relax"] = ([ns.RFPulse(w["quad128"], 4.0, alpha=90, T1=900.0, T2=T2, g=g), ns.ADC], {})
    # phase offset of the whole pulse
    out["phi"] = ([ns.RFPulse(w["sinc64"], 1.5, alpha=70, phi=35.0, T1=700.0, T2=45.0, g=0.2), ns.ADC], {})
    # 6-echo CPMG with shaped refocusing pulses over (2 T2 x 41 positions)
    T2b = np.array([40.0, 120.0])
    exc = ns.encode_phase(ns.RFPulse(w["sinc64"], 2.0, alpha=90, phi=90.0), GRADIENT, FOV, npoint=NPOINT, rewind=True)
    rfc = ns.encode_phase(ns.RFPulse(w["sinc64"], 2.0, alpha=180), GRADIENT, FOV, npoint=NPOINT)
    relax = ns.E(3.0, 1000.0, T2b)
    out["cpmg"] = ([exc] + [relax, ns.S(1), rfc, ns.S(1), relax, ns.ADC] * 6, {})
    return out


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.environ.get("EPGPY_REFERENCE", "/root/reference"))
    if not hasattr(np, "asfarray"):      # (NumPy 2 removed it; the reference's spline helper still calls it)
        np.asfarray = lambda a: np.asarray(a, dtype=np.float64)
    from epgpy import operators, functions, rfpulse, utils  # noqa: E402  (the reference)

    ns = types.SimpleNamespace(RFPulse=rfpulse.RFPulse, encode_phase=rfpulse.encode_phase, estimate_rf=rfpulse.estimate_rf,
                               estimate_alpha=rfpulse.estimate_alpha, spatial_range=utils.spatial_range,
                               space_to_freq=utils.space_to_freq, freq_to_space=utils.freq_to_space,
                               T=operators.T, E=operators.E, S=operators.S, ADC=operators.ADC)
    out = {f"wave_{name}": wave for name, wave in waveforms().items()}
    out.update(host_values(ns))
    for name, (seq, kw) in cases(ns).items():
        F0, Z0 = functions.simulate(seq, probe=("F0", "Z0"), **kw)
        out[name + "_F0"], out[name + "_Z0"] = np.asarray(F0), np.asarray(Z0)
        print(name, out[name + "_F0"].shape, flush=True)
    path = os.path.join(HERE, "g19_rfpulse.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
