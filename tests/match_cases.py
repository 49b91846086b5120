"""Yardstick and seeded cases of the dictionary-matching tests (tests/test_match_host.py on the CPU, tests/test_gpu_match.py).

The yardstick computes n_a, c[a,m] and q[a,m] in np.clongdouble / np.longdouble and holds a float64 result to bounds DERIVED
from the standard inner-product error bound (Higham, Accuracy and Stability, 3.1: |fl(x.y) - x.y| <= gamma_n sum |x_i||y_i|),
with u = 2^-53 and a complex product counted as four real ones -- not to anything measured:

    g        = 4 (nrec + 4) u
    bc[a,m]  = g sum_t |D[t,a]| |S[t,m]|                     bounds |c_dev - c_ref|
    bq[a,m]  = (2 |c| bc + bc^2) / n + g q                   bounds |q_dev - q_ref|  (|c|^2, the norm, the division)

A returned index a* must have q_ref[a*,m] >= max_a q_ref[a,m] - (bq[a*,m] + bq[amax,m]); where the voxel is DECISIVE -- every
other atom (exact copies of the best column apart: these tie bit for bit, and the lowest wins) lies more than twice that sum
below the best -- a* must EQUAL the reference argmax.  scale: |scale n_ref[a*] - c_ref[a*,m]| <= bc + g |c|.  score =
|c| / sqrt(n E), E = sum_t |S[t,m]|^2, is held to the same bound over sqrt(n E), plus g score for the root, quotient and E.
"""
import numpy as np

U = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble


class Yardstick:
    def __init__(self, D, S):
        """D [nrec, natoms], S [nrec, nmeas], complex128"""
        D, S = np.asarray(D, dtype=np.complex128), np.asarray(S, dtype=np.complex128)
        assert D.ndim == 2 and S.ndim == 2 and D.shape[0] == S.shape[0]
        self.D, self.S = D, S
        self.nrec, self.natoms, self.nmeas = D.shape[0], D.shape[1], S.shape[1]
        self.g = LD(4 * (self.nrec + 4) * U)
        with np.errstate(all="ignore"):
            Dl, Sl = D.astype(CLD), S.astype(CLD)
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
        if not self.any_valid:
            return np.zeros(self.nmeas, dtype=bool)
        out = np.zeros(self.nmeas, dtype=bool)
        for m in range(self.nmeas):
            b = self.amax[m]
            copies = np.all(self.D == self.D[:, b:b + 1], axis=0)                                # exact copies of the best column
            others = self.valid & ~copies
            gap = self.q[b, m] - self.q[others, m]
            out[m] = bool(np.all(gap > 2 * (self.bq[others, m] + self.bq[b, m])))
        return out

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
def _cgauss(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def placements(natoms):
    """true atoms worth placing a signal on: first, last, both sides of every 16-atom tile seam, inside the last partial tile,
    both sides of every range boundary for nsplit = 2, 3 (and with it nsplit = natoms: every atom is one)"""
    want = {0, natoms - 1, natoms - 2, natoms // 2}
    for seam in range(16, natoms, 16):
        want |= {seam - 1, seam}
    for nsplit in (2, 3):
        if nsplit <= natoms:
            for lo, _ in split_bounds(natoms, nsplit)[1:]:
                want |= {lo - 1, lo}
    return sorted(a for a in want if 0 <= a < natoms)


def split_bounds(natoms, nsplit):
    """the ranges epgx_signal_match cuts the atoms into (include/epgx.h), restated"""
    q, r = divmod(natoms, nsplit)
    return [(s * q + min(s, r), s * q + min(s, r) + q + (s < r)) for s in range(nsplit)]


def signals_from(D, atoms, rng, noise):
    """S[:, m] = pd_m D[:, atoms[m]] + noise, pd complex"""
    nrec = D.shape[0]
    pd = (0.5 + rng.random(len(atoms))) * np.exp(2j * np.pi * rng.random(len(atoms)))
    scale = np.sqrt(np.mean(np.abs(D) ** 2))
    return pd[None, :] * D[:, atoms] + noise * scale * _cgauss(rng, (nrec, len(atoms)))


def gaussian_case(seed, natoms, nmeas, nrec, noise=0.05):
    """random complex Gaussian dictionary; voxel m is a scaled, noisy copy of atom placements(natoms)[m mod ...]"""
    rng = np.random.default_rng([seed, natoms, nmeas, nrec])
    D = _cgauss(rng, (nrec, natoms))
    place = placements(natoms)
    atoms = np.array([place[m % len(place)] for m in range(nmeas)])
    return D, signals_from(D, atoms, rng, noise), atoms


def decaying_case(seed, natoms, nmeas, nrec, noise=0.01):
    """correlated dictionary: every column a sum of two decaying exponentials with a slow phase roll (neighbouring atoms are
    almost parallel, as in a relaxometry dictionary)"""
    rng = np.random.default_rng([seed, natoms, nmeas, nrec, 7])
    t = np.arange(nrec)[:, None]
    rate = np.geomspace(0.02, 0.6, natoms)[None, :]
    D = (0.7 * np.exp(-rate * t) + 0.3 * np.exp(-0.25 * rate * t)) * np.exp(1j * 0.05 * t * (1 + np.arange(natoms)[None, :] / natoms))
    place = placements(natoms)
    atoms = np.array([place[m % len(place)] for m in range(nmeas)])
    return D, signals_from(D, atoms, rng, noise), atoms


def tie_case():
    """33 atoms, 5 records: atoms 15 and 16 are one column (a pair across the tile seam), atoms 10, 17 and 32 another (a triple
    across the seams and across the range boundary 17 of nsplit = 2).  Voxels lie on all five; the lowest index must come back"""
    D, _, _ = gaussian_case(11, 33, 17, 5)
    D[:, 16] = D[:, 15]
    D[:, 17] = D[:, 10]
    D[:, 32] = D[:, 10]
    rng = np.random.default_rng(12)
    atoms = np.array([16, 15, 32, 17, 10, 0, 31, 16, 32, 17, 15, 10, 16, 32, 17, 5, 20])
    expect = np.where(atoms == 16, 15, np.where((atoms == 17) | (atoms == 32), 10, atoms))
    return D, signals_from(D, atoms, rng, 0.02), expect


def invalid_case():
    """17 atoms, 5 records: atom 3 is all zero, atom 16 holds a NaN, atom 8 an Inf; voxel 4 is an all-zero signal"""
    D, S, atoms = gaussian_case(13, 17, 15, 5)
    D[:, 3] = 0.0
    D[2, 16] = np.nan
    D[1, 8] = np.inf
    S[:, 4] = 0.0
    return D, S, atoms


# (natoms, nmeas, nrec): around the 16 x 16 x 4 tile, the 64-voxel workgroup, the 64-atom pass and the 32-record chunk.
# One record makes every q equal |s|^2 whatever the atom, so nrec = 1 goes with one atom.
SHAPES = [(1, 1, 1), (1, 17, 1), (15, 15, 3), (16, 16, 4), (17, 17, 5), (33, 67, 37), (257, 67, 5), (257, 1, 37), (15, 67, 4),
          (16, 1, 3), (33, 16, 5)]
LONG = (33, 17, 1000)


def cases():
    """name -> (D, S): every case of the GPU tests (the end-to-end run of the simulator apart, which needs the device)"""
    out = {}
    for natoms, nmeas, nrec in SHAPES + [LONG]:
        out[f"gauss_{natoms}_{nmeas}_{nrec}"] = gaussian_case(1, natoms, nmeas, nrec)[:2]
    out["decay_257_67_37"] = decaying_case(2, 257, 67, 37)[:2]
    out["decay_33_17_5"] = decaying_case(2, 33, 17, 5)[:2]
    out["tie"] = tie_case()[:2]
    out["invalid"] = invalid_case()[:2]
    return out
