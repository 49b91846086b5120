"""Shaped RF pulses for the tests: the G19 cases (tests/golden/make_golden_rfpulse.py) and the same pulses EXPANDED into the
oracle's tuples -- ("T", alpha, phi) and ("E", tau, T1, T2, g) / ("P", tau, g) per sample, built here from the waveform, never
from the product's operator list."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_rfpulse as mg  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "g19_rfpulse.npz")
gamma_1H = 42.576 * 1e3


def pulse_tuples(values, duration, rf, *, phi=None, T1=None, T2=None, g=None, slice_freqs=None, rewind=None):
    """the oracle's tuples of RFPulse(values, duration, rf=rf, phi=, T1=, T2=, g=), optionally under a slice-selection gradient
    (`slice_freqs`: kHz, already placed on its grid axis; `rewind`: fraction of the gradient integral rewound afterwards)"""
    values = np.asarray(values, dtype=np.complex128)
    n = len(values)
    tau = duration / n
    out = []
    if phi:
        out.append(("P", 1.0, -phi / 360.0))           # Phi(-phi) = diag(e^{-i phi}, e^{i phi}, 1)
    for v in values:
        out.append(("T", 180 * np.abs(v) * rf, np.angle(v, deg=True)))
        if slice_freqs is not None:
            out.append(("P", tau, slice_freqs))
        if not (T1 is None and T2 is None and g is None):
            out.append(("E", tau, 1e10 if T1 is None else T1, 1e10 if T2 is None else T2, 0 if g is None else g))
    if phi:
        out.append(("P", 1.0, phi / 360.0))
    if rewind is not None:
        out.append(("P", duration * (0.5 if rewind is True else rewind), -slice_freqs))
    return out


def slice_freqs(gradient, fov, npoint, ndim_before=1):
    """the frequency axis encode_phase adds behind `ndim_before` grid axes"""
    freqs = gradient * 1e-6 * gamma_1H * (fov * np.linspace(-0.5, 0.5, npoint))
    return freqs.reshape((1,) * ndim_before + (npoint,))


def sinc_pulse(n, lobes=3):
    x = np.linspace(-lobes, lobes, n)
    return (np.sinc(x) * np.hamming(n)).astype(np.complex128)


def cpmg(epg, necho, T2, *, nsample=32, npoint=9, esp=6.0, shaped_excitation=False):
    """(sequence, oracle tuples) of a CPMG train with a shaped refocusing pulse over (T2 x position); the SAME pulse object
    in every echo"""
    wave = sinc_pulse(nsample)
    T2 = np.asarray(T2, dtype=float)
    pulse = epg.RFPulse(wave, 2.0, alpha=160)
    rfc = epg.encode_phase(pulse, 8.0, 16.0, npoint=npoint)
    relax = epg.E(esp / 2, 1000.0, T2)
    freqs = slice_freqs(8.0, 16.0, npoint)
    rfc_t = pulse_tuples(wave, 2.0, pulse.rf, slice_freqs=freqs)
    relax_t = ("E", esp / 2, 1000.0, T2, 0)
    if shaped_excitation:
        exc_pulse = epg.RFPulse(wave, 2.0, alpha=90, phi=90.0)
        exc = [epg.encode_phase(exc_pulse, 8.0, 16.0, npoint=npoint, rewind=True)]
        exc_t = pulse_tuples(wave, 2.0, exc_pulse.rf, phi=90.0, slice_freqs=freqs, rewind=True)
    else:
        exc, exc_t = [epg.T(90, 90)], [("T", 90, 90)]
    seq = exc + [relax, epg.S(1), rfc, epg.S(1), relax, epg.ADC] * necho
    tuples = exc_t + ([relax_t, ("S", 1)] + rfc_t + [("S", 1), relax_t, ("ADC",)]) * necho
    return seq, tuples


def apply_table(table, state):
    """one order of a state matrix [F0, conj F0, Z0] (density 1) through an EPGX_OP_MAT0 table entry: (F0, Z0) afterwards"""
    u, p, q, t = (table[..., 2 * i] + 1j * table[..., 2 * i + 1] for i in range(4))
    c22, o0, o2 = table[..., 8], table[..., 10] + 1j * table[..., 11], table[..., 12]
    f, z = state[..., 0], state[..., 2]
    f_new = u * f + p * np.conj(f) + q * z + o0
    z_new = t * f + np.conj(t) * np.conj(f) + c22 * z + o2
    return f_new, z_new
