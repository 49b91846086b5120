"""small helpers of the reference's utils module that the hot path's users rely on"""
import enum
import sys

import numpy as np

gamma_1H = 42.576 * 1e3  # kHz/T   (utils.py:8)
gamma_23Na = 11.262 * 1e3  # kHz/T


def Axes(*names):
    """IntEnum of named grid axes, e.g. Axes("FA", "T2") (utils.py:134-145)"""
    return enum.IntEnum("Axes", names, start=0)


def check_states(states):
    """EPG symmetry of a full [*, 2n+1, 3] array (utils.py:118-121)"""
    states = np.asarray(states)
    return np.allclose(states, states[..., ::-1, [1, 0, 2]].conj())


def get_norm(states):
    """utils.py:152-154"""
    states = np.asarray(states)
    return np.sqrt(np.sum(np.abs(states[..., 1:]) ** 2, axis=(-2, -1)))


def get_wavenumber(grad, duration, gamma=gamma_1H):
    """wavenumber (rad/m) of a gradient lobe: mT/m x ms (utils.py:157-169)"""
    return 2 * np.pi * gamma * np.asarray(grad) * 1e-3 * np.asarray(duration)


def spatial_range(fov, nvalue=100):
    """`nvalue` positions across a field of view of `fov` mm, centred (utils.py:175-183)"""
    return fov * np.linspace(-0.5, 0.5, nvalue)


def space_to_freq(grad, positions, *, gamma=gamma_1H):
    """off-resonance frequencies (kHz) of positions (mm) under a gradient (mT/m) (utils.py:186-208)"""
    if not np.isscalar(positions):
        positions = np.asarray(positions)
    return grad * 1e-6 * gamma * positions


def freq_to_space(grad, frequencies, *, gamma=gamma_1H):
    """the reverse of space_to_freq (utils.py:211-213)"""
    return frequencies / grad / gamma * 1e6


def _phasors(theta):
    """exp(i theta) from one cos and one sin per element"""
    out = np.empty(np.shape(theta), dtype=np.complex128)
    np.cos(theta, out=out.real)
    np.sin(theta, out=out.imag)
    return out


def voxel_factor(wavenumbers, voxel_shape="box", voxel_size=1):
    """what a voxel of finite extent does to a phase state of wavenumber k [..., kdim] (rad/m): nothing for a "point",
    prod_d sinc(k_d size_d / 2 pi) for a "box" of `voxel_size` (m, scalar or one per column) -- utils.py:51-61"""
    if voxel_shape == "point":
        return 1.0
    if voxel_shape == "box":
        return np.sinc(np.asarray(wavenumbers) * voxel_size / 2 / np.pi).prod(axis=-1)
    raise ValueError(f"Unknown voxel shape: {voxel_shape}")


def imaging(positions, states, wavenumbers, acctime=None, *, phase=None, weights=None, modulation=None,
            voxel_shape="box", voxel_size=1, expand=True, reduce=True, tol=1e-8):
    """spatial read-out of phase states on host arrays (utils.py:12-95):

        im[..., p] = sum_r  voxel_r mod_r F_r exp(i k_r . x_p)

    positions [*P, d] (1-D: [P, 1]), states F [..., R], wavenumbers k [..., R, kdim] (rad/m), acctime t [..., R] or None.
    `expand`: the position axes are inserted behind the leading axes of F, the result is [..., *P]; otherwise positions
    broadcast against those axes.  Only the first d columns of k enter the phase; the voxel factor runs over all of them
    (`voxel_factor`), and states whose factor is at most `tol` in every voxel are left out.  With `acctime`, `modulation`
    (real part: decay rate, imaginary part: frequency) gives mod = exp(-|t| Re m) exp(2 pi i t Im m), states with mod <= tol
    everywhere left out; `phase` (degrees) multiplies everything.  `weights` multiply the image in place (NumPy
    broadcasting); `reduce`: True sums everything, False keeps everything, an int / tuple sums those axes."""
    F, k = np.asarray(states), np.asarray(wavenumbers)
    t = None if acctime is None else np.asarray(acctime)
    pos = np.asarray(positions)
    if pos.ndim < 2:
        pos = pos[..., np.newaxis]
    if expand:
        extra = pos.ndim - 1
        F = F.reshape(F.shape[:-1] + (1,) * extra + F.shape[-1:])
        k = k.reshape(k.shape[:-2] + (1,) * extra + k.shape[-2:])
        if t is not None:
            t = t.reshape(t.shape[:-1] + (1,) * extra + t.shape[-1:])

    factor = voxel_factor(k, voxel_shape, voxel_size)
    if voxel_shape == "box":
        keep = np.any(np.abs(factor) > tol, axis=tuple(range(F.ndim - 1)))
        F, k, factor = F[..., keep], k[..., keep, :], factor[..., keep]
        if t is not None:
            t = t[..., keep]

    if t is not None:
        m = np.asarray(1.0 if modulation is None else modulation)
        mod = np.exp(-np.abs(t) * m.real[..., np.newaxis])
        keep = np.any(mod > tol, axis=tuple(range(F.ndim - 1)))
        F, k, mod, t = F[..., keep], k[..., keep, :], mod[..., keep], t[..., keep]
        if np.ndim(factor):
            factor = factor[..., keep]
        if np.iscomplexobj(m):
            mod = mod * _phasors(2 * np.pi * t * m.imag[..., np.newaxis])
    else:
        mod = 1.0
    if phase is not None:
        mod = mod * np.exp(1j * np.asarray(phase) * np.pi / 180)

    theta = np.matmul(k[..., : pos.shape[-1]], pos[..., np.newaxis])[..., 0]        # [..., *P, R]
    rows = (factor * mod * F)[..., np.newaxis, :]
    im = np.matmul(rows, _phasors(theta)[..., np.newaxis])[..., 0, 0]
    if weights is not None:
        im *= np.asarray(weights)
    if reduce is True:
        return im.sum()
    if reduce is False:
        return im
    return im.sum(axis=reduce)


def dft(coords, states, wavenumbers, *, reduce=False):
    """`imaging` of point voxels, nothing summed unless asked (utils.py:113-115)"""
    return imaging(coords, states, wavenumbers, reduce=reduce, voxel_shape="point")


class Progress:
    """text progress display behind `simulate(disp=True)` (the reference wraps its operator loop in a progress
    bar, functions.py:175-176 / utils.py:219-236).  Here the unit of progress is a device launch: one per
    ADC-to-ADC segment in the per-timestep mode, one per operator batch in the stepwise mode, a single one for a
    state-resident run -- the bar then jumps from 0 to done when the kernel has finished."""

    def __init__(self, total, prefix="Simulating: ", width=60, out=None):
        self.total, self.prefix, self.width = max(int(total), 1), prefix, width
        self.out = out if out is not None else sys.stdout
        self.done = 0
        self._show()

    def _show(self):
        fill = self.width * self.done // self.total
        print(f"{self.prefix}[{'#' * fill}{'.' * (self.width - fill)}] {self.done}/{self.total}", end="\r", file=self.out, flush=True)

    def step(self, n=1):
        self.done = min(self.total, self.done + n)
        self._show()

    def close(self):
        self.done = self.total
        self._show()
        print("", file=self.out, flush=True)
