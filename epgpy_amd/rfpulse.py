"""Shaped RF pulses and slice profiles (mirrors epgpy/rfpulse.py:37-346).

`RFPulse(values, duration, rf= / alpha=)` models a sampled waveform as a train of small rotations T(alpha_i, phi_i), one per
sample, with relaxation / precession E or P of the sample's duration between them when `T1`, `T2` or `g` are given;
`encode_phase(pulse, gradient, fov)` adds a slice-selection frequency axis.  Names, arguments, return values and exceptions
are the reference's.  Two things differ behind the interface:

  * a pulse whose samples last equally long shares ONE E (or P) object between its samples (the reference's `modify` builds
    one per T): the same values and the same flattened operator list, but one relaxation table on the device instead of N;
  * an RFPulse -- and what `modify` / `encode_phase` make of it -- is flagged `collapsible`: a pulse holds no shift and no
    probe, so `simulate()` has the device multiply its 2 N .. 3 N members up ONCE per voxel and applies the product as one
    operator at every order (collapse.py; `simulate(..., collapse=False)` runs the members one by one).
"""
import logging

import numpy as np

from . import common, evolution, functions, operator, transition, utils

try:
    from scipy import optimize
except ImportError:
    optimize = None

LOGGER = logging.getLogger(__name__)


class RFPulse(operator.MultiOperator):
    """realistic RF-pulse operator (rfpulse.py:37-101)

    values: complex samples of the waveform, magnitudes <= 1; duration: total duration (ms), or one duration per sample;
    rf: RF amplitude (kHz) -- sample i rotates by 180 |values[i]| rf degrees about the axis at angle(values[i]); alpha: target
    flip angle (degrees), reached by estimating `rf`; phi: phase offset of the whole pulse (degrees); T1, T2, g: relaxation
    and off-resonance frequency (kHz) acting during every sample"""

    collapsible = True

    def __init__(self, values, duration, *, rf=None, alpha=None, phi=None, **kwargs):
        seq, info = rfpulse(values, duration, rf=rf, alpha=alpha, phi=phi, **kwargs)
        self.values = values
        for item in info:
            setattr(self, item, info[item])
        name = kwargs.pop("name", f"RFPulse({len(values)}, {duration}ms)")
        super().__init__(seq, name=name, duration=duration)


def shared_modifier():
    """`functions.default_modifier` for the samples of ONE pulse: operators that last equally long receive the same E / P
    object (the parameters are the same for all of them)"""
    shared = {}

    def modifier(op, **kwargs):
        if isinstance(op, transition.T):
            att = kwargs.get("att")
            if att is not None and not np.allclose(att, 1):
                op = transition.T(op.alpha * att, op.phi, name=op.name, duration=op.duration)
                op.name += "#"
        if np.any(op.duration > 0):
            T1, T2, g = kwargs.get("T1"), kwargs.get("T2"), kwargs.get("g")
            if T1 is None and T2 is None and g is None:
                return op
            key = float(op.duration) if np.ndim(op.duration) == 0 else None
            relax = shared.get(key)
            if relax is None:
                if T1 is None and T2 is None:
                    relax = evolution.P(op.duration, g, duration=0)
                else:
                    relax = evolution.E(op.duration, 1e10 if T1 is None else T1, 1e10 if T2 is None else T2,
                                        0 if g is None else g, duration=0)
                if key is not None:
                    shared[key] = relax
            first = op
            op = op * relax
            op.name = first.name + "*"
        return op

    return modifier


def rfpulse(values, duration, rf=None, alpha=None, phi=None, **kwargs):
    """the pulse as a list of operators, and {"rf", "alpha", "phi" [, "T1", "T2", "g"]} (rfpulse.py:104-138)"""
    values = np.asarray(values, dtype=np.complex128)
    if rf is None and alpha is None:
        raise ValueError('Either "rf" or "alpha" must be provided')
    elif rf is None:
        rf = estimate_rf(values, alpha)
    elif alpha is None:
        alpha = estimate_alpha(values, rf)
    # (both given: alpha is only stored)
    transform = kwargs.pop("transform", transition.T)
    seq = make_pulse_sequence(transform, values, duration, rf, offset=phi)
    info = {"rf": rf, "alpha": alpha, "phi": phi}
    T1, T2, g = kwargs.get("T1"), kwargs.get("T2"), kwargs.get("g")
    if not all([T1 is None, T2 is None, g is None]):
        T1 = 1e10 if T1 is None else T1
        T2 = 1e10 if T2 is None else T2
        g = 0 if g is None else g
        seq = functions.modify(seq, shared_modifier(), T1=T1, T2=T2, g=g, expand=False)
        info.update({"T1": T1, "T2": T2, "g": g})
    return seq, info


def make_pulse_sequence(transform, values, duration, rf, offset=None):
    """list of operators from pulse data (rfpulse.py:141-197): values (complex samples), duration (ms, total or per sample),
    rf (kHz), offset (degrees)"""
    values = np.asarray(values)
    if values.ndim > 1:
        raise ValueError("`values` array must be 1-dimensional")
    if np.max(np.abs(values)) > 1:
        raise ValueError("pulse values must have a magnitude <= 1")
    nvalue = len(values)
    ndim = len(np.shape(rf))
    if ndim > 1:
        values = values.reshape((nvalue,) + (1,) * ndim)
    if np.isscalar(duration):
        durations = np.ones(nvalue) * duration / nvalue
    elif len(duration) == nvalue:
        durations = np.asarray(duration)
    else:
        raise ValueError("duration and values must have the same length")
    alphas = 180 * np.abs(values) * rf
    phis = np.angle(values, deg=True)
    sequence = [transform(alpha, phi, duration=dur) for alpha, phi, dur in zip(alphas, phis, durations)]
    if offset:
        sequence = [transition.Phi(-offset)] + sequence + [transition.Phi(offset)]
    return sequence


def _combined_rotation(alphas, phis):
    """product of the small rotations, first sample first (opmatrix.matrix_combine_multi of the reference: the same einsum,
    the same order)"""
    mats = transition.rotation_operator(alphas, phis)
    mat = mats[0]
    for mat_ in mats[1:]:
        mat = np.einsum("...ij,...jk->...ik", mat_, mat)
    return mat


def _rotated_equilibrium(mat):
    """the rotation applied to the equilibrium [0, 0, 1]: [F0, conj F0, Z0] (opmatrix.matrix_prod on a one-row state matrix)"""
    states = np.array([[[0, 0, 1]]], dtype=np.complex128)
    return np.matmul(mat[..., np.newaxis, :, :], states[..., np.newaxis])[..., 0]


def estimate_alpha(values, rf):
    """flip angle (degrees) the waveform reaches at RF amplitude `rf` (rfpulse.py:200-222)"""
    alphas = rf * 180 * np.abs(values)
    phis = np.angle(values, deg=True)
    sim = _rotated_equilibrium(_combined_rotation(alphas, phis))
    absZ = np.mod(np.real(sim.flat[2]) + 1, 2) - 1       # longitudinal coefficient, between -1 and +1
    return np.mod(np.arccos(absZ) / np.pi * 180 + 180, 360) - 180


def estimate_rf(values, alpha):
    """RF amplitude (kHz) that reaches the flip angle `alpha` (rfpulse.py:225-314): closed form for a waveform of constant
    phase, else `scipy.optimize.minimize` on the distance between the rotated equilibrium and that of T(alpha, 90)"""
    values = np.asarray(values)
    if np.max(np.abs(values)) > 1:
        raise ValueError("pulse values must have a magnitude <= 1")
    phase_diffs = np.diff(np.mod(np.angle(values, deg=True), 180))
    if np.all(np.isclose(phase_diffs, 0, atol=1e-5)):
        LOGGER.info(f"Calculate rf for alpha={alpha} (constant phase)")
        return alpha / 180 / np.abs(np.sum(values))
    if not optimize:
        raise RuntimeError("Scipy is required for estimating rf")
    LOGGER.info(f"Optimize rf for alpha={alpha}")
    target = _rotated_equilibrium(transition.rotation_operator(alpha, 90))
    alphas = 180 * np.abs(values)
    phis = np.angle(values, deg=True)

    def costfunction(rf):
        sim = _rotated_equilibrium(_combined_rotation(rf * alphas, phis))
        return np.sum((np.abs(sim) - np.abs(target)) ** 2)

    init = alpha / 180 / np.abs(np.sum(values))
    result = optimize.minimize(costfunction, init, bounds=[(0, None)], tol=1e-8)
    LOGGER.info(result)
    return result.x[0]


def encode_phase(pulse, gradient, fov, *, expand=True, rewind=None, npoint=101, gamma=utils.gamma_1H):
    """the pulse under a slice-selection gradient (mT/m): its positions (`fov` in mm: a width cut into `npoint` positions, or
    the positions themselves) become off-resonance frequencies along a new grid axis (`expand`); `rewind` appends the
    rephasing lobe, as a fraction of the pulse's gradient integral (True: 0.5)  (rfpulse.py:321-346)"""
    if not isinstance(pulse, RFPulse):
        raise TypeError("Can only use RFPulse operators")
    if np.isscalar(fov):
        fov = utils.spatial_range(fov, npoint)
    freqs = utils.space_to_freq(gradient, fov, gamma=gamma)
    if expand:
        freqs = np.expand_dims(freqs, tuple(range(len(pulse.shape))))
    modified = functions.modify(pulse, shared_modifier(), g=freqs, expand=False)
    if rewind is not None:
        rewind = 0.5 if rewind is True else float(rewind)
        modified.append(evolution.P(pulse.duration * rewind, g=-freqs, duration=0))
    return modified
