"""Yardstick and seeded cases of the refinement tests (tests/test_refine_host.py on the CPU, tests/test_gpu_refine.py).

The yardstick computes every accumulator of `match.refine` (n, E, c, b_p, h_p, Re M_pq) in np.clongdouble / np.longdouble and
holds a float64 result to bounds DERIVED from the inner-product bound (Higham, Accuracy and Stability, 3.1) with u = 2^-53 and a
complex product counted as four real ones -- nothing is measured:

    g = 4 (nrec + 4) u        Dn = g sum |d|^2   DE = g sum |s|^2   Dc = g sum |d||s|   Db_p = g sum |j_p||s|
                              Dh_p = g sum |d||j_p|   DM_pq = g sum |j_p||j_q|

and e = 16 u for the handful of roundings that form a quantity from the accumulators.  With n- = n - Dn (> 0, else the voxel is
not checked beyond its flags), A_pq = Re M_pq - Re(conj(h_p) h_q) / n, rho = c / n, t_p = b_p - rho conj(h_p):

    DA_pq   = DM_pq + (|h_p| Dh_q + |h_q| Dh_p + Dh_p Dh_q) / n- + |h_p||h_q| Dn / (n n-) + e (|M_pq| + |h_p||h_q| / n)
    Drho2   = (|c| + Dc)^2 / n-^2 (1 + e) - |rho|^2             (the upper deviation is the larger one)
    DN_pq   = (|rho|^2 + Drho2) DA_pq + Drho2 |A_pq|
    Drho    = (Dc + |rho| Dn) / n- + e |rho|
    Dt_p    = Db_p + |rho| Dh_p + Drho |h_p| + Drho Dh_p + e (|b_p| + |rho||h_p|)
    Dy_p    = |rho| Dt_p + Drho |t_p| + Drho Dt_p + e |rho||t_p|

delta is checked through the residual of the normal equations, not through a condition number: for every resolved voxel and p

    |sum_q N_pq delta_q - y_p| <= sum_q DN_pq |delta_q| + Dy_p + gamma_chol sum_q |N_pq||delta_q|,    gamma_chol = gamma_(3P+1)

(Higham Th. 10.4: the backward error of a P x P Cholesky solve; the equilibration is a diagonal scaling, which a componentwise
relative bound does not see, and its roundings are inside e).  Clipping is checked exactly where the caller hands over the
unclipped result of the same voxels: the clipped delta must be its clip, bit for bit; the residual is then asked of the
unclipped one.  scale' and score' are held to bounds derived the same way from the DEVICE's own delta:

    Dnum = Dc + sum |delta_p| Db_p + e (|c| + sum |delta_p||b_p|)
    Dden = Dn + 2 sum |delta_p| Dh_p + sum |delta_p||delta_q| DM_pq + e (n + 2 sum |delta_p||h_p| + sum |delta_p||delta_q||M_pq|)
    |scale' den - num| <= Dnum + |scale'| Dden + e |num|
    |score' sqrt(den E) - |num|| <= Dnum + score' DX / sqrt(den E) + e |num|,     DX = den DE + E Dden + Dden DE

Unresolved voxels: scale = rho within (Dc + |rho| Dn) / n- + e |rho| and the unrefined score within the bound of match_cases.

Decisiveness.  A voxel is decisive if every yardstick pivot of Nhat is > 1e-6 (it must come back resolved), or if it is BUILT
unresolved: an index outside the atoms, n or an M_pp zero or not finite, an all-zero signal, or some pivot < 1e-13 (a column that
is a multiple of d or of another column, nrec = 1, more real unknowns than 2 nrec - 2).  Voxels in between may go either way.
"""
import numpy as np

from tests import match_cases as mc

U = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble
EPS = LD(16 * U)


def gamma(k):
    return LD(k * U) / (1 - LD(k * U))


class Yardstick:
    def __init__(self, D, J, S, index, rcond=1e-10):
        """D [nrec, natoms], J [nrec, natoms, P], S [nrec, nmeas], index [nmeas]"""
        D, J, S = np.asarray(D, np.complex128), np.asarray(J, np.complex128), np.asarray(S, np.complex128)
        index = np.asarray(index, np.int64)
        self.nrec, self.natoms = D.shape
        self.P, self.nmeas = J.shape[2], S.shape[1]
        assert J.shape[:2] == D.shape and S.shape[0] == self.nrec and index.shape == (self.nmeas,)
        self.index, self.rcond = index, rcond
        P, g = self.P, LD(4 * (self.nrec + 4) * U)
        self.g = g
        self.valid = (index >= 0) & (index < self.natoms)
        at = np.where(self.valid, index, 0)
        with np.errstate(all="ignore"):
            d, j, s = D[:, at].astype(CLD), J[:, at, :].astype(CLD), S.astype(CLD)
            ad, aj, as_ = np.abs(d), np.abs(j), np.abs(s)
            self.n, self.E = (ad ** 2).sum(axis=0), (as_ ** 2).sum(axis=0)
            self.c = (np.conj(d) * s).sum(axis=0)
            self.b = np.einsum("tmp,tm->mp", np.conj(j), s)
            self.h = np.einsum("tm,tmp->mp", np.conj(d), j)
            self.M = np.einsum("tmp,tmq->mpq", np.conj(j), j).real
            self.Dn, self.DE, self.Dc = g * self.n, g * self.E, g * (ad * as_).sum(axis=0)
            self.Db = g * np.einsum("tmp,tm->mp", aj, as_)
            self.Dh = g * np.einsum("tm,tmp->mp", ad, aj)
            self.DM = g * np.einsum("tmp,tmq->mpq", aj, aj)
            n, c, b, h, M = self.n, self.c, self.b, self.h, self.M
            self.mpp = np.einsum("mpp->mp", M)
            self.rho = c / n
            self.rho2 = np.abs(self.rho) ** 2
            ah = np.abs(h)
            self.A = M - (np.conj(h)[:, :, None] * h[:, None, :]).real / n[:, None, None]
            self.N = self.rho2[:, None, None] * self.A
            self.t = b - self.rho[:, None] * np.conj(h)
            self.y = (np.conj(self.rho)[:, None] * self.t).real
            nm = n - self.Dn
            self.nm = nm
            DA = (self.DM + (ah[:, :, None] * self.Dh[:, None, :] + ah[:, None, :] * self.Dh[:, :, None]
                             + self.Dh[:, :, None] * self.Dh[:, None, :]) / nm[:, None, None]
                  + (ah[:, :, None] * ah[:, None, :]) * (self.Dn / (n * nm))[:, None, None]
                  + EPS * (np.abs(M) + ah[:, :, None] * ah[:, None, :] / n[:, None, None]))
            Drho2 = (np.abs(c) + self.Dc) ** 2 / nm ** 2 * (1 + EPS) - self.rho2
            self.DN = (self.rho2 + Drho2)[:, None, None] * DA + Drho2[:, None, None] * np.abs(self.A)
            arho = np.abs(self.rho)
            self.Drho = (self.Dc + arho * self.Dn) / nm + EPS * arho
            Dt = (self.Db + arho[:, None] * self.Dh + self.Drho[:, None] * ah + self.Drho[:, None] * self.Dh
                  + EPS * (np.abs(b) + arho[:, None] * ah))
            at_ = np.abs(self.t)
            self.Dy = arho[:, None] * Dt + self.Drho[:, None] * at_ + self.Drho[:, None] * Dt + EPS * arho[:, None] * at_
            # pivots of Nhat = A / sqrt(M_pp M_qq), by Cholesky in longdouble
            sd = np.sqrt(self.mpp)
            L = self.A / (sd[:, :, None] * sd[:, None, :])
            self.pivots = np.full((self.nmeas, P), np.nan, dtype=LD)
            for q in range(P):
                piv = L[:, q, q] - (L[:, q, :q] ** 2).sum(axis=1)
                self.pivots[:, q] = piv
                L[:, q, q] = np.sqrt(piv)
                for p in range(q + 1, P):
                    L[:, p, q] = (L[:, p, q] - (L[:, p, :q] * L[:, q, :q]).sum(axis=1)) / L[:, q, q]
            sane = np.isfinite(self.n) & (self.n > 0) & np.all(np.isfinite(self.mpp) & (self.mpp > 0), axis=1)
            zero = sane & (self.E == 0)                  # (c is a sum of exact zeros in any arithmetic)
            firm = np.all(np.nan_to_num(self.pivots, nan=-1.0) > 1e-6, axis=1)
            tiny = np.any(np.nan_to_num(self.pivots, nan=1.0) < 1e-13, axis=1)
        self.sane = sane
        self.must_resolve = self.valid & sane & ~zero & firm & (self.rho2 > 0) & np.isfinite(self.rho2)
        self.must_not = ~self.valid | ~sane | zero | tiny
        self.must_resolve &= ~self.must_not
        self.decisive = self.must_resolve | self.must_not

    # -------------------------------------------------------------------------------------------------------------------
    def residual(self, m, delta):
        """(|N delta - y|, its bound, sum |N||delta| + |y|) of voxel m, each [P]"""
        dl = np.asarray(delta, dtype=LD)
        ad = np.abs(dl)
        res = np.abs(self.N[m] @ dl - self.y[m])
        size = np.abs(self.N[m]) @ ad
        bound = self.DN[m] @ ad + self.Dy[m] + gamma(3 * self.P + 1) * size
        return res, bound, size + np.abs(self.y[m])

    def check(self, delta, scale, score, unclipped=None, limit=None, what=""):
        """asserts the result of all voxels (delta [nmeas, P]); returns the largest used shares of the bounds, the decisive share
        and the share of the resolved voxels whose residual bound is <= 1e-6 (sum |N||delta| + |y|)"""
        delta, scale, score = np.asarray(delta), np.asarray(scale).reshape(-1), np.asarray(score).reshape(-1)
        assert delta.shape == (self.nmeas, self.P) and delta.dtype == np.float64
        assert scale.dtype == np.complex128 and score.dtype == np.float64
        free = delta if unclipped is None else np.asarray(unclipped)
        if unclipped is not None:
            lim = np.broadcast_to(np.asarray(limit, dtype=np.float64), (self.P,))
            want = np.where(free > lim, lim, np.where(free < -lim, -lim, free))
            assert want.tobytes() == delta.tobytes(), (what, "the clipped step is not the clip of the unclipped one")
        worst = dict(residual=0.0, scale=0.0, score=0.0)
        resolved = sharp = 0
        with np.errstate(all="ignore"):
            for m in range(self.nmeas):
                tag = f"{what} voxel {m}"
                got = bool(np.isfinite(delta[m]).all())
                assert got or np.isnan(delta[m]).all(), (tag, delta[m])
                if self.must_resolve[m]:
                    assert got, (tag, "must be resolved", self.pivots[m])
                if self.must_not[m]:
                    assert not got, (tag, "must be unresolved", self.pivots[m])
                if not self.valid[m]:
                    assert scale[m] == 0 and score[m] == 0, (tag, scale[m], score[m])
                    continue
                if not self.sane[m] or not self.nm[m] > 0:
                    continue          # (an atom that is zero or holds a NaN: rho and the score are whatever 0 / 0 and NaN give)
                n, E, c = self.n[m], self.E[m], self.c[m]
                if not got:
                    tol = self.Drho[m]
                    err = abs(CLD(scale[m]) - self.rho[m])
                    assert err <= tol, (tag, "scale of an unresolved voxel", float(err), float(tol))
                    if E == 0:
                        assert score[m] == 0.0, (tag, score[m])
                    else:
                        root = np.sqrt(n * E)
                        stol = (self.Dc[m] + self.g * abs(c)) / root + self.g * abs(c) / root
                        serr = abs(LD(score[m]) - abs(c) / root)
                        assert serr <= stol, (tag, "score of an unresolved voxel", float(serr), float(stol))
                    continue
                resolved += 1
                res, bound, size = self.residual(m, free[m])
                assert np.all(res <= bound), (tag, "residual", res.astype(float), bound.astype(float))
                sharp += bool(np.all(bound <= 1e-6 * size))
                worst["residual"] = max(worst["residual"], float(np.max(res / np.where(bound > 0, bound, 1))))
                dl = delta[m].astype(LD)
                ad = np.abs(dl)
                num = c + dl @ self.b[m]
                den = n + 2 * (dl @ self.h[m].real) + dl @ self.M[m] @ dl
                Dnum = self.Dc[m] + ad @ self.Db[m] + EPS * (abs(c) + ad @ np.abs(self.b[m]))
                Dden = (self.Dn[m] + 2 * (ad @ self.Dh[m]) + ad @ self.DM[m] @ ad
                        + EPS * (n + 2 * (ad @ np.abs(self.h[m])) + ad @ np.abs(self.M[m]) @ ad))
                tol = Dnum + abs(scale[m]) * Dden + EPS * abs(num)
                err = abs(CLD(scale[m]) * den - num)
                assert err <= tol, (tag, "scale", float(err), float(tol))
                worst["scale"] = max(worst["scale"], float(err / tol))
                if E == 0:
                    assert score[m] == 0.0, (tag, score[m])
                    continue
                root = np.sqrt(den * E)
                DX = den * self.DE[m] + E * Dden + Dden * self.DE[m]
                stol = Dnum + LD(score[m]) * DX / root + EPS * abs(num)
                serr = abs(LD(score[m]) * root - abs(num))
                assert serr <= stol, (tag, "score", float(serr), float(stol))
                worst["score"] = max(worst["score"], float(serr / stol))
        worst["decisive"] = float(self.decisive.mean())
        worst["sharp"] = sharp / resolved if resolved else 1.0
        return worst


# ---------------------------------------------------------------------------------------------------------- seeded cases
def gaussian_case(seed, natoms, nmeas, nrec, P, noise=0.02, step=0.05):
    """random complex Gaussian dictionary and Jacobian; voxel m is a scaled, noisy copy of the linearised atom
    D[:, a] + J[:, a] delta_m at a = match_cases.placements(natoms)[m mod ...] with |delta| ~ step"""
    rng = np.random.default_rng([seed, natoms, nmeas, nrec, P])
    D = mc._cgauss(rng, (nrec, natoms))
    J = mc._cgauss(rng, (nrec, natoms, P))
    place = mc.placements(natoms)
    atoms = np.array([place[m % len(place)] for m in range(nmeas)], dtype=np.int64)
    delta = step * rng.standard_normal((nmeas, P))
    pd = (0.5 + rng.random(nmeas)) * np.exp(2j * np.pi * rng.random(nmeas))
    S = pd[None, :] * (D[:, atoms] + np.einsum("tmp,mp->tm", J[:, atoms, :], delta)) + noise * mc._cgauss(rng, (nrec, nmeas))
    return D, J, S, atoms


def decay_atoms(rate, nrec, roll=0.05, k=0.25, w=0.7):
    """the atoms of match_cases.decaying_case at the given rates (phase roll `roll` per record) and their analytic derivatives
    with respect to the rate, the roll, the mixing weight w and the rate ratio k: D [nrec, natoms], J [nrec, natoms, 4]"""
    t = np.arange(nrec, dtype=np.float64)[:, None]
    rate = np.asarray(rate, dtype=np.float64)[None, :]
    roll = np.broadcast_to(np.asarray(roll, dtype=np.float64), rate.shape[1:])[None, :]
    phase = np.exp(1j * roll * t)
    fast, slow = np.exp(-rate * t), np.exp(-k * rate * t)
    D = (w * fast + (1 - w) * slow) * phase
    J = np.stack([(-w * t * fast - (1 - w) * k * t * slow) * phase, 1j * t * D, (fast - slow) * phase,
                  -(1 - w) * rate * t * slow * phase], axis=-1)
    return D, J


def decaying_case(seed, natoms, nmeas, nrec, P, noise=1e-3):
    """the correlated dictionary of match_cases.decaying_case with its analytic rate derivative as J (then roll, weight and rate
    ratio for P > 1); voxels lie a fraction of the grid step off their atoms"""
    rng = np.random.default_rng([seed, natoms, nmeas, nrec, P, 7])
    rate = np.geomspace(0.02, 0.6, natoms)
    roll = 0.05 * (1 + np.arange(natoms) / natoms)
    D, J = decay_atoms(rate, nrec, roll)
    place = mc.placements(natoms)
    atoms = np.array([place[m % len(place)] for m in range(nmeas)], dtype=np.int64)
    off = rate[atoms] * (1 + 0.02 * rng.uniform(-1, 1, nmeas))
    pd = (0.5 + rng.random(nmeas)) * np.exp(2j * np.pi * rng.random(nmeas))
    S = pd[None, :] * decay_atoms(off, nrec, roll[atoms])[0] + noise * mc._cgauss(rng, (nrec, nmeas))
    return D, J[:, :, :P], S, atoms


def special_case():
    """17 atoms, 37 records, P = 3, 131 voxels: index holds -1, 0 and natoms - 1; voxel 4 is an all-zero signal; atom 16 holds a
    NaN; column 1 of atom 5 is a multiple of d, column 2 of atom 6 equals its column 0, column 0 of atom 7 is all zero"""
    D, J, S, atoms = gaussian_case(31, 17, 131, 37, 3)
    atoms = atoms.copy()
    atoms[:12] = [-1, 0, 16, 5, 3, 6, 7, -1, 16, 5, 6, 0]
    D[2, 16] = np.nan
    J[:, 5, 1] = (0.3 - 2j) * D[:, 5]
    J[:, 6, 2] = J[:, 6, 0]
    J[:, 7, 0] = 0.0
    S[:, 4] = 0.0
    return D, J, S, atoms


# (natoms, nmeas, nrec, P): natoms 1, 17, 257; nmeas around the wavefront; nrec 1, 2, 5, 37, 1000 and both sides of the slice
# boundaries 16 | 17, 32 | 33, 64 | 65 of refine_slices; P = 1 .. 4
SHAPES = [(1, 1, 1, 1), (1, 63, 2, 1), (17, 64, 5, 2), (17, 65, 5, 4), (257, 131, 37, 3), (17, 131, 16, 4), (17, 63, 17, 3),
          (257, 64, 32, 2), (17, 65, 33, 4), (17, 131, 64, 1), (257, 63, 65, 4), (17, 17, 2, 4), (17, 5, 1, 3)]
LONG = (17, 65, 1000, 4)
LIMIT = [0.04, np.inf, 0.06]          # with steps ~ 0.05 per column: some voxels are clipped and some are not


def cases():
    """name -> dict(D, J, S, index [, rows, limit]).  `rows`: the columns of J the call takes, in this order (a permutation or a
    subset); the yardstick then gets J[:, :, rows]"""
    out = {}
    for natoms, nmeas, nrec, P in SHAPES + [LONG]:
        D, J, S, idx = gaussian_case(1, natoms, nmeas, nrec, P)
        out[f"gauss_{natoms}_{nmeas}_{nrec}_p{P}"] = dict(D=D, J=J, S=S, index=idx)
    for natoms, nmeas, nrec, P in [(257, 131, 37, 1), (17, 65, 37, 2), (257, 63, 65, 3), (17, 64, 1000, 4)]:
        D, J, S, idx = decaying_case(2, natoms, nmeas, nrec, P)
        out[f"decay_{natoms}_{nmeas}_{nrec}_p{P}"] = dict(D=D, J=J, S=S, index=idx)
    D, J, S, idx = gaussian_case(3, 17, 65, 37, 4)
    out["permuted"] = dict(D=D, J=J, S=S, index=idx, rows=[2, 0, 3, 1])
    out["subset"] = dict(D=D, J=J, S=S, index=idx, rows=[3, 1])
    D, J, S, idx = special_case()
    out["special"] = dict(D=D, J=J, S=S, index=idx)
    D, J, S, idx = gaussian_case(4, 17, 131, 37, 3)
    out["limit"] = dict(D=D, J=J, S=S, index=idx, limit=LIMIT)
    return out


def yardstick(case):
    J = case["J"] if "rows" not in case else case["J"][:, :, case["rows"]]
    return Yardstick(case["D"], J, case["S"], case["index"])
