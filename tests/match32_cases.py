"""Yardstick and seeded cases of the single-precision matching tests (tests/test_match32_host.py on the CPU,
tests/test_gpu_match32.py).

A complex64 dictionary is DEFINED as the complex128 one rounded once, and matching on the rounded operands D32 = fl32(D),
S32 = fl32(S) (include/epgx.h).  The yardstick therefore rounds both operands with `astype(np.complex64)` first -- that rounding
is part of the definition, not an error -- and computes n_a, c[a,m] and q[a,m] of the ROUNDED operands in np.clongdouble /
np.longdouble.  A device result is held to bounds DERIVED as in tests/match_cases.py (Higham, Accuracy and Stability, 3.1:
|fl(x.y) - x.y| <= gamma_n sum |x_i||y_i|, a complex product counted as four real ones), with the unit roundoff of float32,
u = 2^-24, because c is accumulated in float32 -- not to anything measured:

    g        = 4 (nrec + 4) 2^-24
    bc[a,m]  = g sum_t |D32[t,a]| |S32[t,m]|                 bounds |c_dev - c_ref|
    bq[a,m]  = (2 |c| bc + bc^2) / n + g q                   bounds |q_dev - q_ref|

The f32 MFMA is a plain fmaf chain, so the gamma bound holds whatever the order inside an instruction.  Index, "decisive", scale
and score rules are those of match_cases.Yardstick.  The norms are accumulated in float64 on the device and are held to the
FLOAT64 bound 4 (nrec + 4) 2^-53 n.
"""
import numpy as np

from tests import match_cases as mc

U32 = 2.0 ** -24
U64 = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble
CHUNK = 64           # records of one LDS chunk of match32_kernel (csrc/epgx_signal_limits.h MATCH32_CHUNK)
KSTEP = 4            # records one v_mfma_f32_16x16x4_f32 consumes


def fl32(A):
    """the definition's rounding: per component to nearest even, subnormals kept, overflow to +-Inf"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(A, dtype=np.complex128).astype(np.complex64)


class Yardstick32:
    def __init__(self, D, S):
        """D [nrec, natoms], S [nrec, nmeas]: complex128 (rounded here) or complex64 already"""
        D32, S32 = fl32(D), fl32(S)
        assert D32.ndim == 2 and S32.ndim == 2 and D32.shape[0] == S32.shape[0]
        self.D, self.S = D32, S32
        self.nrec, self.natoms, self.nmeas = D32.shape[0], D32.shape[1], S32.shape[1]
        self.g = LD(4 * (self.nrec + 4) * U32)
        self.gn = LD(4 * (self.nrec + 4) * U64)                 # the norms: accumulated in float64
        with np.errstate(all="ignore"):
            Dl, Sl = D32.astype(CLD), S32.astype(CLD)
            self.n = (Dl.real ** 2 + Dl.imag ** 2).sum(axis=0)                                   # [natoms]
            self.valid = np.isfinite(self.n) & (self.n > 0)
            Dv = np.where(self.valid[None, :], Dl, 0)
            nv = np.where(self.valid, self.n, 1)
            self.c = np.einsum("ta,tm->am", np.conj(Dv), Sl)                                     # [natoms, nmeas]
            self.absc = np.abs(self.c)
            self.q = np.where(self.valid[:, None], self.absc ** 2 / nv[:, None], -np.inf)
            self.bc = self.g * np.einsum("ta,tm->am", np.abs(Dv), np.abs(Sl))
            self.bq = (2 * self.absc * self.bc + self.bc ** 2) / nv[:, None] + self.g * np.abs(self.q)
            self.energy = (Sl.real ** 2 + Sl.imag ** 2).sum(axis=0)                              # [nmeas]
        self.nv = nv
        self.any_valid = bool(self.valid.any())
        self.amax = np.argmax(self.q, axis=0) if self.any_valid else np.full(self.nmeas, -1)     # (the lowest among equal q)
        self.decisive = self._decisive()

    def _decisive(self):
        out = np.zeros(self.nmeas, dtype=bool)
        if not self.any_valid:
            return out
        for m in range(self.nmeas):
            b = self.amax[m]
            copies = np.all(self.D == self.D[:, b:b + 1], axis=0)                                # exact copies of the best column
            others = self.valid & ~copies
            gap = self.q[b, m] - self.q[others, m]
            out[m] = bool(np.all(gap > 2 * (self.bq[others, m] + self.bq[b, m])))
        return out

    def check_norms(self, norms):
        """float64 norms of the valid atoms within the float64 bound; invalid atoms are not finite numbers > 0"""
        norms = np.asarray(norms).reshape(self.natoms)
        assert norms.dtype == np.float64
        err = np.abs(norms[self.valid].astype(LD) - self.n[self.valid])
        assert np.all(err <= self.gn * self.n[self.valid]), float(np.max(err / (self.gn * self.n[self.valid])))
        bad = norms[~self.valid]
        assert not np.any(np.isfinite(bad) & (bad > 0)), bad
        return float(np.max(err / (self.gn * self.n[self.valid]))) if self.valid.any() else 0.0

    def check_slack(self, index, what=""):
        """only: the returned atom is valid and its q lies within the slack of the best"""
        index = np.asarray(index).reshape(self.nmeas)
        worst = 0.0
        for m in range(self.nmeas):
            a, b = int(index[m]), int(self.amax[m])
            assert 0 <= a < self.natoms and self.valid[a], (what, m, a)
            slack = self.bq[a, m] + self.bq[b, m]
            short = self.q[b, m] - self.q[a, m]
            assert short <= slack, (what, m, a, b, float(short), float(slack))
            if slack > 0:
                worst = max(worst, float(short / slack))
        return worst

    def check(self, index, scale, score, what=""):
        """asserts the device result of all voxels; returns the largest used fractions of the bounds (for printing)"""
        index, scale, score = (np.asarray(x).reshape(self.nmeas) for x in (index, scale, score))
        assert index.dtype == np.int64 and scale.dtype == np.complex128 and score.dtype == np.float64
        worst = dict(q=0.0, scale=0.0, score=0.0)
        for m in range(self.nmeas):
            tag = f"{what} voxel {m}"
            a = int(index[m])
            if not self.any_valid or not np.isfinite(self.q[self.amax[m], m]):
                assert a == -1 and scale[m] == 0 and score[m] == 0, (tag, a, scale[m], score[m])
                continue
            b = int(self.amax[m])
            assert 0 <= a < self.natoms and self.valid[a], (tag, a)
            slack = self.bq[a, m] + self.bq[b, m]
            short = self.q[b, m] - self.q[a, m]
            assert short <= slack, (tag, a, b, float(short), float(slack))
            if slack > 0:
                worst["q"] = max(worst["q"], float(short / slack))
            if self.decisive[m]:
                assert a == b, (tag, "decisive", a, b)
            tol = self.bc[a, m] + self.g * self.absc[a, m]
            err = abs(CLD(scale[m]) * self.n[a] - self.c[a, m])
            assert err <= tol, (tag, "scale", float(err), float(tol))
            if tol > 0:
                worst["scale"] = max(worst["scale"], float(err / tol))
            assert 0.0 <= score[m] <= 1.0, (tag, score[m])
            if self.energy[m] == 0:
                assert score[m] == 0.0, (tag, score[m])
                continue
            root = np.sqrt(self.n[a] * self.energy[m])
            ref = self.absc[a, m] / root
            stol = tol / root + self.g * ref
            serr = abs(LD(score[m]) - min(ref, LD(1)))
            assert serr <= stol, (tag, "score", float(serr), float(stol))
            if stol > 0:
                worst["score"] = max(worst["score"], float(serr / stol))
        return worst


# ---------------------------------------------------------------------------------------------------------- seeded cases
# 33 atoms x 17 voxels around the LDS chunk of CHUNK records (one chunk less one, one chunk, one more, two chunks and one) and
# one record count that is no multiple of the MFMA's k step
CHUNK_SHAPES = [(33, 17, CHUNK - 1), (33, 17, CHUNK), (33, 17, CHUNK + 1), (33, 17, 2 * CHUNK + 1), (33, 17, KSTEP + 2)]


def cases():
    """name -> (D, S) complex128: every case that is held to the yardstick with the decisive rule (>= 90 % of the voxels of each
    are decisive at float32: tests/test_match32_host.py)"""
    out = {}
    for natoms, nmeas, nrec in mc.SHAPES + [mc.LONG] + CHUNK_SHAPES:
        out[f"gauss_{natoms}_{nmeas}_{nrec}"] = mc.gaussian_case(1, natoms, nmeas, nrec)[:2]
    out["decay_33_67_37"] = mc.decaying_case(2, 33, 67, 37)[:2]
    out["decay_65_67_37"] = mc.decaying_case(2, 65, 67, 37)[:2]
    out["tie"] = mc.tie_case()[:2]
    out["invalid"] = mc.invalid_case()[:2]
    return out


def close_case():
    """decay_257_67_37 of tests/match_cases.py: neighbouring atoms are closer than the float32 bound, NO voxel of it is decisive;
    only the slack rule applies (Yardstick32.check_slack)"""
    return mc.decaying_case(2, 257, 67, 37)[:2]


def narrow_values(shape, seed=5):
    """complex128 values that exercise the rounding: +-0, float32 subnormals, halfway cases (ties to even, both ways), values
    just above FLT_MAX (-> Inf), values just below the overflow threshold, Inf and NaN, among Gaussians"""
    rng = np.random.default_rng([seed, *shape])
    n = int(np.prod(shape))
    fmax = float(np.finfo(np.float32).max)
    special = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -151, 2.0 ** -127, 1.5 * 2.0 ** -140,
                        1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 - 2.0 ** -25, -(1.0 + 2.0 ** -24),
                        fmax, fmax * (1 + 2.0 ** -25), fmax * (1 + 2.0 ** -24), np.nextafter(fmax * (1 + 2.0 ** -25), 0), -fmax * 1.01,
                        1e300, -1e300, np.inf, -np.inf, np.nan, 1e-300])
    re = rng.standard_normal(n)
    im = rng.standard_normal(n)
    k = min(n, len(special))
    re[:k] = special[:k]                     # every special value as a real part (next to another one) ...
    im[:k] = special[:k][::-1]
    im[n - k:] = special[:k]                 # ... and as an imaginary part (next to a Gaussian where the array is long enough)
    out = np.empty(n, dtype=np.complex128)   # (re + 1j * im would turn an Inf into a NaN)
    out.real, out.imag = re, im
    return out.reshape(shape)
